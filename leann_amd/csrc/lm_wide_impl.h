// lm_wide_impl.h -- the wide form of the canonical row distance (d_padded in {1536, 2048, 2560, 3072, 4096}: nch = d_padded / 64 in
// {24, 32, 40, 48, 64}), the kernels of its own (k_dist_pairs_wide, k_exact_scan_wide) and the launchers of every kernel that takes it.
// Included at the end of lm_search.hip; lm_beam_common.h declares wide_stage_query / wide_dist for k_update and k_search_table, which select
// them with NCH == 0 (one instantiation per (metric, dtype), the width is a run-time value).
//
// Why a form of its own: the register-resident form keeps float4 qv[NCH] and two rows float4 e[NCH] per lane -- 3 x 192 VGPRs at nch = 48.
// Here the query sits in LDS, staged once per workgroup (16 nch float4 = d_padded x 4 bytes, 6 .. 16 KB; the four 16-lane groups of a wave
// read the same addresses: a broadcast), and a row streams through registers in blocks of WIDE_BLK = 8 chunks: the block's 8 loads of every
// row in flight are issued first (16-byte loads of fp32 rows, 8-byte loads of fp16 rows), then the block's 8 query float4 are read from
// LDS, then the 32 fmaf per row run in chunk order.  Budget per lane: 64 VGPRs of row data (two rows), 32 of query, 8 accumulators.
// Workgroup (256-thread) kernels only.
#pragma once

namespace lm {

constexpr int WIDE_BLK = 8;  // chunks per block; every wide nch is a multiple

// the block's 8 chunks of one row: lane t of the row's 16 lanes owns float4 chunk c at row[16 c + t]; fp16 rows are widened exactly
template <bool F16>
__device__ __forceinline__ void wide_load_block(const void* table, int64_t first, float4 (&e)[WIDE_BLK]) {
    if (F16) {
        const uint2* p = (const uint2*)table + first;
        uint2 h[WIDE_BLK];
#pragma unroll
        for (int i = 0; i < WIDE_BLK; ++i) h[i] = p[16 * i];
#pragma unroll
        for (int i = 0; i < WIDE_BLK; ++i) {
            const float2 f0 = __half22float2(__builtin_bit_cast(__half2, h[i].x)), f1 = __half22float2(__builtin_bit_cast(__half2, h[i].y));
            e[i] = make_float4(f0.x, f0.y, f1.x, f1.y);
        }
    } else {
        const float4* p = (const float4*)table + first;
#pragma unroll
        for (int i = 0; i < WIDE_BLK; ++i) e[i] = p[16 * i];
    }
}

// one block's 32 fmaf onto the row's four accumulators, in chunk order
template <bool L2>
__device__ __forceinline__ void wide_fma_block(const float4 (&e)[WIDE_BLK], const float4 (&qv)[WIDE_BLK], float (&a)[4]) {
#pragma unroll
    for (int i = 0; i < WIDE_BLK; ++i) {
        if (L2) {
            const float d0 = e[i].x - qv[i].x, d1 = e[i].y - qv[i].y, d2 = e[i].z - qv[i].z, d3 = e[i].w - qv[i].w;
            a[0] = __builtin_fmaf(d0, d0, a[0]);
            a[1] = __builtin_fmaf(d1, d1, a[1]);
            a[2] = __builtin_fmaf(d2, d2, a[2]);
            a[3] = __builtin_fmaf(d3, d3, a[3]);
        } else {
            a[0] = __builtin_fmaf(e[i].x, qv[i].x, a[0]);
            a[1] = __builtin_fmaf(e[i].y, qv[i].y, a[1]);
            a[2] = __builtin_fmaf(e[i].z, qv[i].z, a[2]);
            a[3] = __builtin_fmaf(e[i].w, qv[i].w, a[3]);
        }
    }
}

// lane sum and the 16-lane butterfly of row_reduce
template <bool L2>
__device__ __forceinline__ float wide_finish(const float (&a)[4]) {
    float s = (a[0] + a[1]) + (a[2] + a[3]);
    s += __shfl_xor(s, 8, 16);
    s += __shfl_xor(s, 4, 16);
    s += __shfl_xor(s, 2, 16);
    s += __shfl_xor(s, 1, 16);
    return L2 ? s : -s;
}

// query q of Q [.][64 nch] -> sq[0 .. 16 nch), by the nt threads of the workgroup; the caller's next barrier publishes it
__device__ __forceinline__ void wide_stage_query(const float* Q, int64_t q, int nch, float4* sq, int tid, int nt) {
    const float4* qrow = (const float4*)(Q + (size_t)q * 64 * (size_t)nch);
    for (int i = tid; i < 16 * nch; i += nt) sq[i] = qrow[i];
}

// Distances of ROWS rows (slot = row of `table`, stride 64 nch elements) to the query at qrow (16 nch float4, in LDS or in global memory), by the
// 16 lanes of a group.  BIT FOR BIT row_reduce<NCH> (== oracle/lm_oracle.c:orc_dist): row_reduce runs ONE fmaf chain per float4 component over
// the lane's chunks in ascending order, starting from 0; the chain does not know where a block ends, so a loop that carries the four
// accumulators from block to block performs the same sequence of roundings -- and the lane sum and the butterfly are the same expressions.
template <bool L2, bool F16, int ROWS>
__device__ __forceinline__ void wide_dist(const void* table, const int64_t (&slot)[ROWS], const float4* qrow, int nch, int lane16, float (&dist)[ROWS]) {
    float acc[ROWS][4];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) acc[r][0] = acc[r][1] = acc[r][2] = acc[r][3] = 0.f;
#pragma unroll 1
    for (int c = 0; c < nch; c += WIDE_BLK) {
        float4 e[ROWS][WIDE_BLK], qv[WIDE_BLK];
#pragma unroll
        for (int r = 0; r < ROWS; ++r) wide_load_block<F16>(table, slot[r] * (int64_t)(16 * nch) + 16 * c + lane16, e[r]);
#pragma unroll
        for (int i = 0; i < WIDE_BLK; ++i) qv[i] = qrow[16 * (c + i) + lane16];
#pragma unroll
        for (int r = 0; r < ROWS; ++r) wide_fma_block<L2>(e[r], qv, acc[r]);
    }
#pragma unroll
    for (int r = 0; r < ROWS; ++r) dist[r] = wide_finish<L2>(acc[r]);
}

// lm_dist_gather at a wide width: as k_dist_pairs, 16 pairs per workgroup.  Every pair names its own query, so the queries stay in global
// memory (16 x 16 KB would not fit the LDS; a pair reads its query once).
template <bool L2, bool F16>
__global__ __launch_bounds__(256) void k_dist_pairs_wide(const void* table, const float* Q, const int32_t* qidx, const int32_t* ids, int64_t npairs, int nch,
                                                         float* out) {
    const int lane16 = threadIdx.x & 15;
    const int64_t p = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    if (p >= npairs) return;
    const int64_t slot[1] = {ids[p]};
    float d[1];
    wide_dist<L2, F16, 1>(table, slot, (const float4*)(Q + (size_t)qidx[p] * 64 * (size_t)nch), nch, lane16, d);
    if (lane16 == 0) out[p] = d[0];
}

// k_exact_scan at a wide width: the same (row slice, query tile) grid, lists, thresholds, pending lists and flushes (exact_flush), one row per
// 16-lane group and step.  Eight queries of 4096 floats do not fit the LDS next to the lists, so the tile's queries are walked in sub-tiles
// of QS (8 up to 2048 wide, else 4: at most 64 KB of queries) and the slice's rows are read again for every sub-tile.  A row block is loaded
// once and scored against the sub-tile's queries, 4 accumulators per query; a (row, query) distance is wide_dist's chain whatever sub-tile
// it falls in, and the lists are per query: labels and distance bits do not depend on the sub-tiling.
// dynamic LDS: queries[QS][16 nch] (float4) | lists[qalloc][2][k] | cand[qalloc][EXACT_CAP]
template <bool L2, bool F16, int QS>
__global__ __launch_bounds__(256) void k_exact_scan_wide(const void* table, int64_t ntable, const float* Q, int64_t nq, int k, const uint32_t* allow, int S,
                                                         int64_t rows_per_slice, int qalloc, int nch, uint64_t* part) {
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ int s_cnt[EXACT_QT], s_np[EXACT_QT], s_cur[EXACT_QT], s_flag[2];
    __shared__ uint64_t s_thr[EXACT_QT];
    constexpr int LIMIT = EXACT_CAP - 16;  // a step appends at most 16 keys per query
    const int tid = threadIdx.x, lane16 = tid & 15, g = tid >> 4;
    const int s = (int)(blockIdx.x % (unsigned)S);
    const int64_t q0 = (int64_t)(blockIdx.x / (unsigned)S) * EXACT_QT;
    const int nqh = (int)min((int64_t)EXACT_QT, nq - q0);
    float4* sq = (float4*)smem;
    uint64_t* lists = (uint64_t*)(sq + (size_t)QS * nch * 16);
    uint64_t* cand = lists + (size_t)qalloc * 2 * k;
    if (tid < EXACT_QT) {
        s_cnt[tid] = 0;
        s_np[tid] = 0;
        s_cur[tid] = 0;
        s_thr[tid] = KEY_NONE;
    }
    if (tid < 2) s_flag[tid] = 0;
    const int64_t lo = (int64_t)s * rows_per_slice, hi = min(ntable, lo + rows_per_slice);
    int par = 0;
    for (int sub = 0; sub < nqh; sub += QS) {
        const int nqs = min(QS, nqh - sub);
        __syncthreads();  // the sub-tile before this one has been read to its end
        const float4* qsrc = (const float4*)(Q + (size_t)(q0 + sub) * 64 * (size_t)nch);
        for (int i = tid; i < nqs * nch * 16; i += 256) sq[i] = qsrc[i];
        __syncthreads();
        for (int64_t base = lo; base < hi; base += 16, par ^= 1) {
            const int64_t row = base + g;
            const bool valid = row < hi && (allow == nullptr || ((allow[row >> 5] >> (row & 31)) & 1u));  // the same for the 16 lanes of a group
            float acc[QS][4];
#pragma unroll
            for (int q = 0; q < QS; ++q) acc[q][0] = acc[q][1] = acc[q][2] = acc[q][3] = 0.f;
            if (valid) {
#pragma unroll 1
                for (int c = 0; c < nch; c += WIDE_BLK) {
                    float4 e[WIDE_BLK];
                    wide_load_block<F16>(table, row * (int64_t)(16 * nch) + 16 * c + lane16, e);
#pragma unroll
                    for (int q = 0; q < QS; ++q) {
                        if (q < nqs) {
                            float4 qv[WIDE_BLK];
#pragma unroll
                            for (int i = 0; i < WIDE_BLK; ++i) qv[i] = sq[q * (16 * nch) + 16 * (c + i) + lane16];
                            wide_fma_block<L2>(e, qv, acc[q]);
                        }
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < QS; ++q) {
                if (q < nqs) {
                    const float d = wide_finish<L2>(acc[q]);  // (every lane of the workgroup: a skipped row reduces its zeros)
                    if (lane16 == 0 && valid) {
                        const uint64_t key = make_key(d, (int32_t)row);
                        if (key < s_thr[sub + q]) {  // rejected against the k-th key before any insertion work
                            const int pos = atomicAdd(&s_cnt[sub + q], 1);
                            cand[(sub + q) * EXACT_CAP + pos] = key;
                            if (pos + 1 > LIMIT) atomicAdd(&s_flag[par], 1);
                        }
                    }
                }
            }
            __syncthreads();
            if (s_flag[par]) {  // written in this step only, read after its barrier: the same for every thread
                for (int q = 0; q < nqh; ++q)
                    exact_flush(lists + (size_t)q * 2 * k, k, cand + q * EXACT_CAP, &s_cnt[q], &s_np[q], &s_cur[q], &s_thr[q], tid);
                if (tid == 0) s_flag[par] = 0;
                __syncthreads();
            }
        }
    }
    __syncthreads();
    for (int q = 0; q < nqh; ++q) exact_flush(lists + (size_t)q * 2 * k, k, cand + q * EXACT_CAP, &s_cnt[q], &s_np[q], &s_cur[q], &s_thr[q], tid);
    __syncthreads();
    for (int q = 0; q < nqh; ++q) {
        const uint64_t* src = lists + (size_t)q * 2 * k + s_cur[q] * k;
        uint64_t* dst = part + ((size_t)(q0 + q) * S + s) * k;
        const int np = s_np[q];
        for (int j = tid; j < k; j += 256) dst[j] = j < np ? src[j] : KEY_NONE;
    }
}

}  // namespace lm

// ---- host side --------------------------------------------------------------------------------------------------------------------------

// k_update<0, ..>: the three addressing modes at 256 threads (option update_variant = 3 is served by them: the same bits from both forms)
#define LAUNCH_UPDATE_WIDE(l2, f16)                                                                                                       \
    do {                                                                                                                                  \
        if (a.by_rank == 2) hipLaunchKernelGGL((k_update<0, l2, f16, 2, 256>), grid, block, shmem, ix->stream, ix->ws, a);                \
        else if (a.by_rank) hipLaunchKernelGGL((k_update<0, l2, f16, 1, 256>), grid, block, shmem, ix->stream, ix->ws, a);                \
        else hipLaunchKernelGGL((k_update<0, l2, f16, 0, 256>), grid, block, shmem, ix->stream, ix->ws, a);                               \
    } while (0)
static int launch_update_wide(lm_index* ix, UpdateArgs a, bool f16) {
    a.nch = ix->Dp / 64;
    const size_t shmem = (size_t)(2 * ix->ws.ef + std::max(next_pow2(ix->ws.maxnew), 2)) * sizeof(uint64_t) + (size_t)ix->Dp * 4;
    if (shmem > 64 * 1024) LM_FAIL(LM_EINVAL, LOCKSTEP_LDS_TEXT);  // (search_lds_checks has refused it before anything was allocated)
    const dim3 grid(ix->ws.B), block(256);
    const bool l2 = ix->metric == LM_METRIC_L2;
    if (l2 && f16) LAUNCH_UPDATE_WIDE(true, true);
    else if (l2) LAUNCH_UPDATE_WIDE(true, false);
    else if (f16) LAUNCH_UPDATE_WIDE(false, true);
    else LAUNCH_UPDATE_WIDE(false, false);
    LM_HIP(hipGetLastError());
    return LM_OK;
}
#undef LAUNCH_UPDATE_WIDE

// k_search_table<0, .., 256, GraphDev> (a view index has no wide width; option persistent_wave = 1 is served by this form)
#define LAUNCH_PERSIST_WIDE(l2, f16)                                                                                                      \
    do {                                                                                                                                  \
        static DynLdsAttr attr;                                                                                                           \
        LM_HIP(ensure_dyn_lds(attr, (const void*)k_search_table<0, l2, f16, 256, GraphDev>, shmem));                                      \
        hipLaunchKernelGGL((k_search_table<0, l2, f16, 256, GraphDev>), dim3(ix->ws.B), dim3(256), shmem, ix->stream, g, ix->ws, a);      \
    } while (0)
static int launch_persist_wide(lm_index* ix, PersistArgs a, const GraphDev& g, size_t shmem) {
    const bool l2 = ix->metric == LM_METRIC_L2, f16 = ix->table_dtype == LM_DTYPE_F16;
    if (l2 && f16) LAUNCH_PERSIST_WIDE(true, true);
    else if (l2) LAUNCH_PERSIST_WIDE(true, false);
    else if (f16) LAUNCH_PERSIST_WIDE(false, true);
    else LAUNCH_PERSIST_WIDE(false, false);
    LM_HIP(hipGetLastError());
    return LM_OK;
}
#undef LAUNCH_PERSIST_WIDE

static int launch_dist_pairs_wide(const void* d_table, bool f16, int32_t d_padded, bool l2, const float* d_q, const int32_t* d_qidx, const int32_t* d_ids,
                                  int64_t npairs, float* d_out, hipStream_t st) {
    const dim3 grid((unsigned)((npairs + 15) / 16)), block(256);
    const int nch = d_padded / 64;
    if (l2 && f16) hipLaunchKernelGGL((k_dist_pairs_wide<true, true>), grid, block, 0, st, d_table, d_q, d_qidx, d_ids, npairs, nch, d_out);
    else if (l2) hipLaunchKernelGGL((k_dist_pairs_wide<true, false>), grid, block, 0, st, d_table, d_q, d_qidx, d_ids, npairs, nch, d_out);
    else if (f16) hipLaunchKernelGGL((k_dist_pairs_wide<false, true>), grid, block, 0, st, d_table, d_q, d_qidx, d_ids, npairs, nch, d_out);
    else hipLaunchKernelGGL((k_dist_pairs_wide<false, false>), grid, block, 0, st, d_table, d_q, d_qidx, d_ids, npairs, nch, d_out);
    LM_HIP(hipGetLastError());
    return LM_OK;
}

template <bool L2, bool F16, int QS>
static int launch_exact_scan_wide_qs(const void* d_table, int64_t ntable, int32_t d_padded, const float* d_q, int64_t nq, int32_t k, const uint32_t* d_allow,
                                     const ExactPlan& p, uint64_t* part, hipStream_t st) {
    static DynLdsAttr attr;
    const int qalloc = (int)std::min<int64_t>(EXACT_QT, nq);
    const size_t shmem = (size_t)QS * d_padded * 4 + (size_t)qalloc * (2 * (size_t)k * 8 + EXACT_CAP * 8);  // at most 64 KB + 36 KB
    LM_HIP(ensure_dyn_lds(attr, (const void*)k_exact_scan_wide<L2, F16, QS>, shmem));
    hipLaunchKernelGGL((k_exact_scan_wide<L2, F16, QS>), dim3((unsigned)(p.S * p.nqt)), dim3(256), shmem, st, d_table, ntable, d_q, nq, (int)k, d_allow,
                       (int)p.S, p.rows, qalloc, d_padded / 64, part);
    return LM_OK;
}

static int launch_exact_scan_wide(const void* d_table, bool f16, int64_t ntable, int32_t d_padded, bool l2, const float* d_q, int64_t nq, int32_t k,
                                  const uint32_t* d_allow, const ExactPlan& p, uint64_t* part, hipStream_t st) {
#define GOW(QS)                                                                                                                   \
    (l2 ? (f16 ? launch_exact_scan_wide_qs<true, true, QS>(d_table, ntable, d_padded, d_q, nq, k, d_allow, p, part, st)           \
               : launch_exact_scan_wide_qs<true, false, QS>(d_table, ntable, d_padded, d_q, nq, k, d_allow, p, part, st))         \
        : (f16 ? launch_exact_scan_wide_qs<false, true, QS>(d_table, ntable, d_padded, d_q, nq, k, d_allow, p, part, st)          \
               : launch_exact_scan_wide_qs<false, false, QS>(d_table, ntable, d_padded, d_q, nq, k, d_allow, p, part, st)))
    return d_padded <= 2048 ? GOW(8) : GOW(4);
#undef GOW
}
