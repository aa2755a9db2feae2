// lm_rc_parts.h -- the built-in recompute provider's part planner (lm_recompute.hip): which chunk ranges of one forward run as concurrent
// lanes.  Pure host functions over plain integers: no HIP, no allocation, so a stand-alone program checks them under the sanitizers
// (tests/rc_parts/rc_parts_check.cpp).
//
// A decision unit is one forward of the provider: n chunks with cumulative token counts cu[0] = 0 <= cu[1] <= ... <= cu[n] = total.
// For `lanes` lanes the length scan (k_rc_lengths_scan) reports lanes - 1 split points: split point j (1 <= j < lanes) is the first chunk i
// with cu[i + 1] > j * total / lanes, together with cu[i] -- both in one 64-bit word, so the host learns each part's chunk range AND its
// token count from the copy that already carries the round's total.  A unit of zero tokens has no such chunk: the point is (n, total).
// Part p is the chunk range [point p, point p + 1) with point 0 = 0 and point `lanes` = n.  The unit is split only if EVERY part holds
// more than lane_min_tokens tokens; otherwise it stays one forward (one part empty -- a 256-token chunk among 1-token chunks --, a
// unit too small to fill the chip several times).
#pragma once
#include <cstdint>

namespace lm {

constexpr int RC_MAX_LANES = 3;

struct RcPart {
    int32_t b0 = 0;      // first chunk of the part (index into the unit's list)
    int32_t n = 0;       // chunks
    int64_t tokens = 0;  // cu[b0 + n] - cu[b0]
};

inline unsigned long long rc_split_pack(int32_t index, int64_t cu_at_index) { return ((unsigned long long)(uint32_t)cu_at_index << 32) | (uint32_t)index; }
inline int32_t rc_split_index(unsigned long long w) { return (int32_t)(uint32_t)w; }
inline int64_t rc_split_tokens(unsigned long long w) { return (int64_t)(w >> 32); }

// the split points as the scan kernel defines them, from cumulative lengths on the host (the reference of the kernel's second pass)
inline void rc_split_points(const int32_t* cu, int32_t n, int lanes, unsigned long long* out /* [lanes - 1] */) {
    const int64_t total = n > 0 ? (int64_t)cu[n] : 0;
    for (int j = 1; j < lanes; ++j) {
        const int64_t thr = (int64_t)j * total / lanes;
        int32_t i = 0;
        while (i < n && (int64_t)cu[i + 1] <= thr) ++i;
        out[j - 1] = rc_split_pack(i, i < n ? (int64_t)cu[i] : total);
    }
}

// parts of one unit of n chunks / total tokens -> out[0 .. return value); 1 = the unit runs as one forward.  Split points that are out
// of order or out of range (a stale or foreign counter block) leave the unit whole as well.
inline int rc_plan_parts(int32_t n, int64_t total, int lanes, int64_t lane_min_tokens, const unsigned long long* split, RcPart* out /* [RC_MAX_LANES] */) {
    out[0].b0 = 0;
    out[0].n = n;
    out[0].tokens = total;
    if (lanes < 2 || lanes > RC_MAX_LANES || n < lanes || !split || lane_min_tokens < 0 || total <= lane_min_tokens * lanes) return 1;
    RcPart p[RC_MAX_LANES];
    int32_t b = 0;
    int64_t t = 0;
    for (int j = 0; j < lanes; ++j) {
        const int32_t e = j + 1 < lanes ? rc_split_index(split[j]) : n;
        const int64_t te = j + 1 < lanes ? rc_split_tokens(split[j]) : total;
        if (e <= b || e > n || te - t <= lane_min_tokens || te > total) return 1;
        p[j].b0 = b;
        p[j].n = e - b;
        p[j].tokens = te - t;
        b = e;
        t = te;
    }
    for (int j = 0; j < lanes; ++j) out[j] = p[j];
    return lanes;
}

}  // namespace lm
