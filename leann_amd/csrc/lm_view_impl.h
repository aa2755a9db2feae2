// lm_view_impl.h -- the dense-level graph accessor of k_search_table: an lm_index that is a live VIEW of device-resident level
// adjacencies in lm_graph_add_links' layout (lm_index_create_view; include/leann_mi355x.h states the contract).
// Part of lm_search.hip's translation unit (included there in front of lm_kernels_persist.h, whose kernel takes the accessor as a
// template parameter; the host side -- creation, guards, launch -- is in lm_search.hip).
//
// Reference surface replaced: none in the reference (faiss searches its own HNSW object while it builds, hnsw_backend.py:66-94);
// here it replaces the per-batch CSR re-assembly of leann_amd/gpu_graph_build.py (temp_csr -> Mi355xIndex.from_csr -> search -> close).
//
// What differs from the CSR accessor (nbr_range / g.l0[...] / g.neighbors[...]):
//   upper-level step   the row of `cur` is its position in the level's sorted node list (binary search, the same in every lane: a
//                      uniform chain of ~log2(n_rows) loads); the row's cap slots are read coalesced and the non-empty ones are
//                      compacted into s_new with the ballot / popcount scheme of the level-0 hop; a node the level does not list has
//                      no neighbours and no row is touched;
//   level-0 hop        every popped node contributes exactly cap slots, so slot f of the flattened range belongs to pop f / cap and
//                      no offset scan is needed; an empty slot (a value outside [0, N)) is not fresh and never reaches the visited
//                      bitmap.
// Everything after the new-list is the CSR kernel's code.
#pragma once

#include <type_traits>

namespace lm {

struct ViewLevelDev {  // one upper level (device array, entry l - 1 = level l)
    const int32_t* nodes;  // n_rows ids, ascending; NULL = identity
    const int32_t* adj;    // [n_rows][cap]
    int32_t n_rows, cap;
};

struct ViewDev {
    int64_t N;
    int32_t entry_point, max_level;
    const int32_t* adj0;  // level 0: [N][cap0], row r = node r
    int32_t cap0;
    const ViewLevelDev* up;
};

template <class GA>
struct graph_is_view : std::false_type {};
template <>
struct graph_is_view<ViewDev> : std::true_type {};

__device__ __forceinline__ bool view_id_ok(int32_t v, int64_t n) { return v >= 0 && (int64_t)v < n; }

// neighbours of `node` at upper level `level` -> s_new[0 .. return value), in slot order.  Called by all NT threads of the workgroup
// (it contains barriers); the row lookup gives every thread the same answer, so the early return is taken by all or by none.
template <int NT>
__device__ __forceinline__ int view_upper_list(const ViewDev& g, int32_t node, int level, int32_t* s_new, int* s_wcnt, int tid) {
    const ViewLevelDev L = g.up[level - 1];
    int64_t row = -1;
    if (!L.nodes) {
        if (node < L.n_rows) row = node;
    } else {
        int lo = 0, hi = L.n_rows;
        while (lo < hi) {
            const int mid = (int)(((int64_t)lo + hi) >> 1);
            if (L.nodes[mid] < node) lo = mid + 1;
            else hi = mid;
        }
        if (lo < L.n_rows && L.nodes[lo] == node) row = lo;
    }
    if (row < 0) return 0;
    const int32_t* arow = L.adj + row * (int64_t)L.cap;
    const int lane = tid & 63, wv = tid >> 6;
    int total = 0;
    for (int c0 = 0; c0 < L.cap; c0 += NT) {
        const int c = c0 + tid;
        int32_t v = -1;
        if (c < L.cap) v = arow[c];
        const bool ok = view_id_ok(v, g.N);
        const unsigned long long m = __ballot(ok);
        if (lane == 0) s_wcnt[wv] = __popcll(m);
        __syncthreads();
        int woff = 0;
        for (int i = 0; i < wv; ++i) woff += s_wcnt[i];
        if (ok) s_new[total + woff + __popcll(m & ((1ull << lane) - 1ull))] = v;
        for (int i = 0; i < NT / 64; ++i) total += s_wcnt[i];
        __syncthreads();
    }
    return total;
}

}  // namespace lm
