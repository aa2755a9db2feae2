// rc_parts_check.cpp -- stand-alone check of the recompute provider's part planner (leann_amd/csrc/lm_rc_parts.h): hand-made cumulative
// lengths -> split points -> part ranges.  No GPU, no library: build with -fsanitize=address,undefined and run (tests/test_rc_parts.py).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../leann_amd/csrc/lm_rc_parts.h"

using namespace lm;

static int g_failed = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++g_failed;                                                 \
        }                                                               \
    } while (0)

static std::vector<int32_t> cumulative(const std::vector<int32_t>& len) {
    std::vector<int32_t> cu(len.size() + 1, 0);
    for (size_t i = 0; i < len.size(); ++i) cu[i + 1] = cu[i] + len[i];
    return cu;
}

// plans one unit from its lengths; checks what every plan must satisfy: the parts tile [0, n) in order, their tokens add up to the
// total, each holds more than lane_min tokens, and the split points are the first chunks past j total / lanes
static int plan(const std::vector<int32_t>& len, int lanes, int64_t lane_min, RcPart* out) {
    const std::vector<int32_t> cu = cumulative(len);
    const int32_t n = (int32_t)len.size();
    const int64_t total = cu[n];
    unsigned long long split[2] = {~0ull, ~0ull};
    rc_split_points(cu.data(), n, lanes, split);
    for (int j = 1; j < lanes; ++j) {
        const int32_t i = rc_split_index(split[j - 1]);
        const int64_t thr = (int64_t)j * total / lanes;
        CHECK(i >= 0 && i <= n);
        if (i < n) {
            CHECK(cu[i + 1] > thr && cu[i] <= thr);
            CHECK(rc_split_tokens(split[j - 1]) == cu[i]);
        } else {
            CHECK(total == 0 && rc_split_tokens(split[j - 1]) == total);
        }
    }
    const int np = rc_plan_parts(n, total, lanes, lane_min, split, out);
    CHECK(np == 1 || np == lanes);
    int32_t b = 0;
    int64_t t = 0;
    for (int p = 0; p < np; ++p) {
        CHECK(out[p].b0 == b && out[p].n >= (np > 1 ? 1 : 0));
        CHECK(out[p].tokens == (int64_t)cu[out[p].b0 + out[p].n] - cu[out[p].b0]);
        if (np > 1) CHECK(out[p].tokens > lane_min);
        b += out[p].n;
        t += out[p].tokens;
    }
    CHECK(b == n && t == total);
    return np;
}

int main() {
    RcPart p[RC_MAX_LANES];
    for (int lanes = 1; lanes <= RC_MAX_LANES; ++lanes) {
        CHECK(plan({}, lanes, 256, p) == 1);                           // an empty call
        CHECK(plan({0, 0, 0, 0, 0, 0}, lanes, 256, p) == 1);           // every chunk empty
        CHECK(plan({200}, lanes, 16, p) == 1);                         // one chunk cannot be split
        CHECK(plan({200, 200}, 3, 16, p) == 1);                        // fewer chunks than lanes
        CHECK(plan(std::vector<int32_t>(600, 100), 1, 256, p) == 1);   // one lane never splits
    }
    // exact multiples: 600 chunks of 100 tokens
    CHECK(plan(std::vector<int32_t>(600, 100), 2, 256, p) == 2);
    CHECK(p[0].n == 300 && p[1].b0 == 300 && p[1].n == 300 && p[0].tokens == 30000 && p[1].tokens == 30000);
    CHECK(plan(std::vector<int32_t>(600, 100), 3, 256, p) == 3);
    CHECK(p[0].n == 200 && p[1].b0 == 200 && p[1].n == 200 && p[2].b0 == 400 && p[2].n == 200 && p[2].tokens == 20000);
    // the chunk that straddles the threshold goes to the later part: {3, 3, 3} at 2 lanes -> thr 4 -> {3} | {3, 3}
    CHECK(plan({3, 3, 3}, 2, 2, p) == 2);
    CHECK(p[0].n == 1 && p[0].tokens == 3 && p[1].n == 2 && p[1].tokens == 6);
    // empty chunks at a boundary stay with the earlier part (the split point is the first chunk that crosses the threshold)
    CHECK(plan({4, 0, 0, 4}, 2, 1, p) == 2);
    CHECK(p[0].n == 3 && p[0].tokens == 4 && p[1].b0 == 3 && p[1].n == 1);
    // just below / at / above lane_min_tokens: every part must hold MORE than it
    CHECK(plan({1024, 1024}, 2, 1024, p) == 1);
    CHECK(plan({1025, 1025}, 2, 1024, p) == 2);
    CHECK(plan({1025, 1024}, 2, 1024, p) == 1);
    CHECK(plan(std::vector<int32_t>(30, 103), 3, 1024, p) == 3);  // 3090 tokens: 1030 each
    CHECK(plan(std::vector<int32_t>(30, 102), 3, 1024, p) == 1);  // 3060 tokens: 1020 each
    // an equal-token split that would leave a part empty: one 256-token chunk in front of / behind 1-token chunks
    {
        std::vector<int32_t> len(101, 1);
        len[0] = 256;
        CHECK(plan(len, 2, 0, p) == 1);  // the first chunk alone crosses half of 356: part 0 would be empty
        len[0] = 1;
        len[100] = 256;
        CHECK(plan(len, 2, 0, p) == 2);  // 100 one-token chunks | the long one
        CHECK(p[0].n == 100 && p[0].tokens == 100 && p[1].n == 1 && p[1].tokens == 256);
        CHECK(plan(len, 2, 256, p) == 1);  // ... but not when a part must hold more than 256 tokens
        CHECK(plan(len, 3, 0, p) == 1);    // both thirds' thresholds fall into the long chunk: the middle part would be empty
    }
    // split words that do not describe this unit (stale counters, a foreign block) leave it whole
    {
        RcPart q[RC_MAX_LANES];
        unsigned long long bad[2] = {rc_split_pack(700, 100), rc_split_pack(5, 50)};
        CHECK(rc_plan_parts(600, 60000, 3, 256, bad, q) == 1 && q[0].b0 == 0 && q[0].n == 600 && q[0].tokens == 60000);
        unsigned long long order[2] = {rc_split_pack(400, 40000), rc_split_pack(200, 20000)};
        CHECK(rc_plan_parts(600, 60000, 3, 256, order, q) == 1);
        unsigned long long over[2] = {rc_split_pack(300, 70000), 0};
        CHECK(rc_plan_parts(600, 60000, 2, 256, over, q) == 1);
        CHECK(rc_plan_parts(600, 60000, 2, 256, nullptr, q) == 1);
        CHECK(rc_plan_parts(600, 60000, 4, 256, order, q) == 1);  // more lanes than the planner has
    }
    // a large unit: 2^31 - 1 tokens fit the 32-bit halves of a split word
    {
        const unsigned long long w = rc_split_pack(INT32_MAX, INT32_MAX);
        CHECK(rc_split_index(w) == INT32_MAX && rc_split_tokens(w) == INT32_MAX);
    }
    if (g_failed) {
        std::printf("%d check(s) failed\n", g_failed);
        return 1;
    }
    std::printf("RC-PARTS-OK\n");
    return 0;
}
