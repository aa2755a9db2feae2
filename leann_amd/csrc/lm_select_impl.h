// lm_select_impl.h -- index build time: the select-neighbours heuristic (Malkov & Yashunin Alg. 4 = faiss shrink_neighbor_list; the
// LEANN paper's Alg. 3 calls the same rule) with Vamana's relaxed second pass (DiskANN occlude_list), as ONE kernel over all rows.
// Included at the end of lm_search.hip (shares load_row / row_reduce: every pairwise distance is the canonical reduction of
// oracle/lm_oracle.c:orc_dist, so the keep mask is a function of the inputs' bits alone; tests/select_ref/lm_select_ref.c restates it).
//
// Reference surface replaced: index.hnsw.efConstruction / index.add of leann_backend_hnsw/hnsw_backend.py:66-94 (faiss picks every
// node's links with this rule while it inserts), leann_amd/gpu_graph_build.py's torch form of it.
//
// Shape: one 16-lane group per row -- the canonical reduction's width -- so four rows per wavefront, 16 per workgroup, no LDS and no
// barrier.  The scan is sequential in j; candidate j sits in registers and the rows kept so far stream past it through L2 until one
// dominates it.  The kept set is a K-bit mask that every lane of the group holds (after the xor butterfly all 16 lanes own the same
// distance, so they take the same decision).  DESIGN.md (kernel list) has the measurement behind this choice.
#pragma once

namespace lm {

constexpr int SELECT_WORDS = LM_SELECT_MAX_K / 64;

template <int NCH, bool L2, bool F16>
__global__ __launch_bounds__(256) void k_select_neighbors(const void* table, int64_t ntable, const int32_t* cand, const float* dist, int64_t n,
                                                          int K, int m, float a2, int relaxed, uint8_t* keep) {
    const int lane16 = threadIdx.x & 15;
    const int64_t r = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    if (r >= n) return;  // a whole 16-lane group leaves together
    const int32_t* c = cand + r * K;
    const float* dj = dist + r * K;
    uint64_t kept[SELECT_WORDS];
#pragma unroll
    for (int w = 0; w < SELECT_WORDS; ++w) kept[w] = 0;
    int cnt = 0;
    float4 cv[NCH], e[NCH];
    for (int pass = 0; pass <= relaxed; ++pass) {
        for (int j = 0; j < K && cnt < m; ++j) {
            const int32_t cj = c[j];
            if (cj < 0 || (int64_t)cj >= ntable) continue;  // empty slot: never kept, never dereferenced
            bool mine = false;
#pragma unroll
            for (int w = 0; w < SELECT_WORDS; ++w) mine |= (j >> 6) == w && ((kept[w] >> (j & 63)) & 1ull);
            if (mine) continue;  // (relaxed pass: kept by the strict one)
            float thr = dj[j];
            if (pass) thr = L2 ? thr / a2 : -(1.0f - (1.0f + thr) / a2);
            load_row<NCH, F16>(table, cj, lane16, cv);
            bool dominated = false;
#pragma unroll
            for (int w = 0; w < SELECT_WORDS; ++w) {
                uint64_t bits = kept[w];
                while (bits && !dominated) {
                    const int i = w * 64 + __builtin_ctzll(bits);
                    bits &= bits - 1;
                    load_row<NCH, F16>(table, c[i], lane16, e);  // kept ids passed the bound check when they were kept
                    if (row_reduce<NCH, L2>(e, cv) <= thr) dominated = true;  // plain IEEE: NaN never dominates
                }
            }
            if (!dominated) {
#pragma unroll
                for (int w = 0; w < SELECT_WORDS; ++w)
                    if ((j >> 6) == w) kept[w] |= 1ull << (j & 63);
                ++cnt;
            }
        }
    }
    for (int j = lane16; j < K; j += 16) {
        uint64_t word = 0;
#pragma unroll
        for (int w = 0; w < SELECT_WORDS; ++w)
            if ((j >> 6) == w) word = kept[w];
        keep[r * K + j] = (uint8_t)((word >> (j & 63)) & 1ull);
    }
}

// what lm_select_neighbors rejects before it looks at a buffer
inline int select_check_params(int32_t dtype, int64_t ntable, int32_t d_padded, int32_t metric, int64_t n, int32_t K, int32_t m, float alpha) {
    if (d_padded <= 0 || d_padded % 64) LM_FAIL(LM_EINVAL, "d_padded must be a positive multiple of 64");
    if (K < 1 || K > LM_SELECT_MAX_K) LM_FAIL(LM_EINVAL, "K must be in [1, LM_SELECT_MAX_K = " + std::to_string(LM_SELECT_MAX_K) + "]");
    if (m < 1) LM_FAIL(LM_EINVAL, "m must be >= 1");
    if (!std::isfinite(alpha) || alpha < 1.0f) LM_FAIL(LM_EINVAL, "alpha must be finite and >= 1");
    if (n < 0 || ntable < 0) LM_FAIL(LM_EINVAL, "n / ntable must not be negative");
    if (dtype != LM_DTYPE_F32 && dtype != LM_DTYPE_F16) LM_FAIL(LM_EINVAL, "dtype must be f32 or f16");
    if (metric != LM_METRIC_INNER_PRODUCT && metric != LM_METRIC_L2) LM_FAIL(LM_EINVAL, "unknown metric");
    switch (d_padded / 64) {
        case 1: case 2: case 3: case 4: case 5: case 6: case 8: case 12: case 16: break;
        default: LM_FAIL(LM_EINVAL, "unsupported padded dimension (supported: 64..384, 512, 768, 1024)");
    }
    if ((n + 15) / 16 > 0x7fffffffll) LM_FAIL(LM_EINVAL, "n too large for one launch");
    return LM_OK;
}

// the launch of lm_select_neighbors on checked arguments (n >= 1): both it and lm_graph_insert_batch (lm_insert_impl.h) enqueue exactly this
inline int select_launch(const void* d_table, int32_t dtype, int64_t ntable, int32_t d_padded, int32_t metric, const int32_t* d_cand, const float* d_dist, int64_t n,
                         int32_t K, int32_t m, float alpha, uint8_t* d_keep, hipStream_t st) {
    const float a2 = alpha * alpha;
    const int relaxed = alpha != 1.0f ? 1 : 0;
    dim3 grid((unsigned)((n + 15) / 16)), block(256);
    const bool l2 = metric == LM_METRIC_L2, f16 = dtype == LM_DTYPE_F16;
#define GO(nch)                                                                                                                                  \
    case nch:                                                                                                                                    \
        if (l2 && f16) hipLaunchKernelGGL((k_select_neighbors<nch, true, true>), grid, block, 0, st, d_table, ntable, d_cand, d_dist, n, K, m, a2, relaxed, d_keep);   \
        else if (l2) hipLaunchKernelGGL((k_select_neighbors<nch, true, false>), grid, block, 0, st, d_table, ntable, d_cand, d_dist, n, K, m, a2, relaxed, d_keep);    \
        else if (f16) hipLaunchKernelGGL((k_select_neighbors<nch, false, true>), grid, block, 0, st, d_table, ntable, d_cand, d_dist, n, K, m, a2, relaxed, d_keep);   \
        else hipLaunchKernelGGL((k_select_neighbors<nch, false, false>), grid, block, 0, st, d_table, ntable, d_cand, d_dist, n, K, m, a2, relaxed, d_keep);           \
        break
    switch (d_padded / 64) {
        GO(1); GO(2); GO(3); GO(4); GO(5); GO(6); GO(8); GO(12); GO(16);
    }
#undef GO
    LM_HIP(hipGetLastError());
    return LM_OK;
}

}  // namespace lm

extern "C" {

int lm_select_neighbors(const void* d_table, int32_t dtype, int64_t ntable, int32_t d_padded, int32_t metric, const int32_t* d_cand,
                        const float* d_dist, int64_t n, int32_t K, int32_t m, float alpha, uint8_t* d_keep, void* stream) {
    using namespace lm;
    if (int rc = select_check_params(dtype, ntable, d_padded, metric, n, K, m, alpha)) return rc;
    if (n == 0) return LM_OK;
    if (!d_cand || !d_dist || !d_keep || (ntable > 0 && !d_table)) LM_FAIL(LM_EINVAL, "NULL buffer");
    return select_launch(d_table, dtype, ntable, d_padded, metric, d_cand, d_dist, n, K, m, alpha, d_keep, (hipStream_t)stream);
}

}  // extern "C"
