// lm_exact_impl.h -- exact top-k over a stored-embedding table: oracle/lm_oracle.c:orc_bruteforce_topk (the paper's IndexFlatIP baseline) plus an
// allow-list, as two kernels.  Included at the end of lm_search.hip (shares load_row / row_reduce / make_key / rank_merge_unsorted: every
// (query, row) distance is the canonical reduction of orc_dist and the ranking is the (distance, id) key of every traversal kernel, so labels AND
// distance bits are a function of the inputs' bits alone).
//
// Reference surface: the reference has no exact path of its own -- it filters AFTER the graph search (leann/api.py:785-790: metadata_filters), so a
// filtered query returns fewer than top_k hits; an exact scan takes the allow-list for free and always returns the best top_k of the allowed rows.
//
// k_exact_scan   one 256-thread workgroup per (row slice, tile of EXACT_QT = 8 queries).  16 groups of 16 lanes -- the canonical reduction's width; a
//                group loads R rows (2 up to 384 dimensions, else 1) into registers ONCE and scores them against every query of the tile (the queries
//                sit in LDS).  Per query the workgroup keeps a sorted top-k key list in LDS and its k-th key as the threshold: a (row, query) pair
//                whose key is not below it costs one comparison.  Survivors are appended to a per-query pending list (EXACT_CAP = 64 keys; an LDS
//                integer counter hands out the places -- the ORDER inside the pending list is not fixed, the SET is, and the merge ranks by key);
//                when a pending list could overflow in the next step the workgroup merges it into the top-k list (rank_merge_unsorted: one barrier).
//                One barrier per step otherwise (the "merge now" flag alternates between two words, so that a fast wave of step i + 1 cannot change
//                what a slow wave of step i reads).  The slice's list goes to the workspace: part[(query * S + slice) * k + j], KEY_NONE = empty.
// k_exact_merge  one workgroup per query: the S sorted partial lists stream past the same threshold / pending list / merge (EXACT_MCAP = 1024
//                pending keys, 512 keys per step), seeded with slice 0's list; writes labels and distances.  (lm_topk_merge holds all S k keys in
//                LDS and stops at 2048 of them.)
// No float atomics, nothing depends on which workgroup finishes first.
//
// Slicing policy -- a pure function of (ntable, nq): exact_plan().
//     nqt  = max(1, ceil(nq / 8))                        query tiles
//     s0   = clamp(ceil(ntable / 1024), 1, max(1, 512 / nqt))
//     rows = max(32, ceil(ntable / s0) rounded up to a multiple of 32)      rows per slice
//     S    = max(1, ceil(ntable / rows))                 slices; the last one holds ntable - (S - 1) rows
// One query: ntable <= 1024 is one slice, 1025 .. 2048 two, 20 000 twenty (19 of 1024 rows and a last one of 544), 1M rows 505 slices of 1984.
// LDS of the scan: 8 queries x d_padded x 4 B + 8 x 2 x k x 8 B (the list and the list being merged into) + 8 x 64 x 8 B, with min(8, nq) in place of
// 8: 6 KB for one 384-wide query at k = 256, 68 KB at the limits (eight 1024-wide queries, k = 256).  Merge: 2 x 256 x 8 + 1024 x 8 = 12 KB.
#pragma once

namespace lm {

constexpr int EXACT_QT = 8;             // queries per tile
constexpr int EXACT_SLICE_ROWS = 1024;  // no slice is cut smaller than this (except the last)
constexpr int EXACT_TARGET_WG = 512;    // slices x query tiles the policy aims for
constexpr int EXACT_CAP = 64;           // scan: pending keys per query
constexpr int EXACT_MCAP = 1024;        // merge: pending keys
constexpr int EXACT_MSTEP = 512;        // merge: keys read per step

struct ExactPlan {
    int64_t nqt, S, rows;
};
static ExactPlan exact_plan(int64_t ntable, int64_t nq) {
    ExactPlan p;
    p.nqt = std::max<int64_t>(1, (nq + EXACT_QT - 1) / EXACT_QT);
    const int64_t smax = std::max<int64_t>(1, EXACT_TARGET_WG / p.nqt);
    const int64_t s0 = std::min(smax, std::max<int64_t>(1, (ntable + EXACT_SLICE_ROWS - 1) / EXACT_SLICE_ROWS));
    p.rows = std::max<int64_t>(32, ((ntable + s0 - 1) / s0 + 31) / 32 * 32);
    p.S = std::max<int64_t>(1, (ntable + p.rows - 1) / p.rows);
    return p;
}

// pending keys cand[0 .. *cnt) into the sorted list (two buffers of k keys at `lists`, *cur names the live one).  Every thread of the workgroup calls it
// between two barriers that no thread has passed while *cnt could still change; ends with a barrier when it had work, thread 0's updates of the four
// words become visible at the caller's next barrier.
__device__ __forceinline__ void exact_flush(uint64_t* lists, int k, const uint64_t* cand, int* cnt, int* np, int* cur, uint64_t* thr, int tid) {
    const int n = *cnt, np0 = *np, c = *cur;
    if (n == 0) return;  // the same for every thread
    uint64_t* dst = lists + (c ^ 1) * k;
    rank_merge_unsorted<256>(lists + c * k, np0, cand, n, dst, k, tid);
    if (tid == 0) {
        const int np1 = min(k, np0 + n);
        *np = np1;
        *cnt = 0;
        *cur = c ^ 1;
        *thr = np1 == k ? dst[k - 1] : KEY_NONE;
    }
}

template <int NCH, bool L2, bool F16, int R>
__global__ __launch_bounds__(256) void k_exact_scan(const void* table, int64_t ntable, const float* Q, int64_t nq, int k, const uint32_t* allow, int S,
                                                    int64_t rows_per_slice, int qalloc, uint64_t* part) {
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ int s_cnt[EXACT_QT], s_np[EXACT_QT], s_cur[EXACT_QT], s_flag[2];
    __shared__ uint64_t s_thr[EXACT_QT];
    constexpr int LIMIT = EXACT_CAP - 16 * R;  // a step appends at most 16 R keys per query
    const int tid = threadIdx.x, lane16 = tid & 15, g = tid >> 4;
    const int s = (int)(blockIdx.x % (unsigned)S);
    const int64_t q0 = (int64_t)(blockIdx.x / (unsigned)S) * EXACT_QT;
    const int nqh = (int)min((int64_t)EXACT_QT, nq - q0);
    float4* sq = (float4*)smem;                                      // qalloc x NCH x 16
    uint64_t* lists = (uint64_t*)(sq + (size_t)qalloc * NCH * 16);   // qalloc x 2 x k
    uint64_t* cand = lists + (size_t)qalloc * 2 * k;                 // qalloc x EXACT_CAP
    const float4* qsrc = (const float4*)(Q + (size_t)q0 * (NCH * 64));
    for (int i = tid; i < nqh * NCH * 16; i += 256) sq[i] = qsrc[i];
    if (tid < EXACT_QT) {
        s_cnt[tid] = 0;
        s_np[tid] = 0;
        s_cur[tid] = 0;
        s_thr[tid] = KEY_NONE;
    }
    if (tid < 2) s_flag[tid] = 0;
    __syncthreads();
    const int64_t lo = (int64_t)s * rows_per_slice, hi = min(ntable, lo + rows_per_slice);
    int par = 0;
    for (int64_t base = lo; base < hi; base += 16 * R, par ^= 1) {
        float4 e[R][NCH];
        bool valid[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int64_t row = base + g * R + r;
            valid[r] = row < hi && (allow == nullptr || ((allow[row >> 5] >> (row & 31)) & 1u));  // the same for the 16 lanes of a group
            if (valid[r]) {
                load_row<NCH, F16>(table, row, lane16, e[r]);
            } else {
#pragma unroll
                for (int i = 0; i < NCH; ++i) e[r][i] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
        for (int q = 0; q < nqh; ++q) {
            float4 qv[NCH];
#pragma unroll
            for (int i = 0; i < NCH; ++i) qv[i] = sq[q * (NCH * 16) + lane16 + 16 * i];
            const uint64_t thr = s_thr[q];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const float d = row_reduce<NCH, L2>(e[r], qv);
                if (lane16 == 0 && valid[r]) {
                    const uint64_t key = make_key(d, (int32_t)(base + g * R + r));
                    if (key < thr) {  // rejected against the k-th key before any insertion work
                        const int pos = atomicAdd(&s_cnt[q], 1);
                        cand[q * EXACT_CAP + pos] = key;
                        if (pos + 1 > LIMIT) atomicAdd(&s_flag[par], 1);  // (several lanes may say so in one step)
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
    for (int q = 0; q < nqh; ++q) exact_flush(lists + (size_t)q * 2 * k, k, cand + q * EXACT_CAP, &s_cnt[q], &s_np[q], &s_cur[q], &s_thr[q], tid);
    __syncthreads();
    for (int q = 0; q < nqh; ++q) {
        const uint64_t* src = lists + (size_t)q * 2 * k + s_cur[q] * k;
        uint64_t* dst = part + ((size_t)(q0 + q) * S + s) * k;
        const int np = s_np[q];
        for (int j = tid; j < k; j += 256) dst[j] = j < np ? src[j] : KEY_NONE;
    }
}

__global__ __launch_bounds__(256) void k_exact_merge(const uint64_t* part, int S, int k, int metric, float* dist, int64_t* labels) {
    __shared__ uint64_t s_list[2 * LM_EXACT_MAX_K];
    __shared__ uint64_t s_cand[EXACT_MCAP];
    __shared__ int s_cnt, s_np, s_cur, s_flag[2];
    __shared__ uint64_t s_thr;
    constexpr int LIMIT = EXACT_MCAP - EXACT_MSTEP;
    const int tid = threadIdx.x;
    const uint64_t* in = part + (size_t)blockIdx.x * S * k;
    const int64_t total = (int64_t)S * k;
    if (tid == 0) {
        s_cnt = 0;
        s_np = 0;
        s_cur = 0;
        s_flag[0] = s_flag[1] = 0;
    }
    __syncthreads();
    for (int j = tid; j < k; j += 256) {  // slice 0's list seeds the result: sorted, its empty places at the end
        const uint64_t key = in[j];
        s_list[j] = key;
        if (key != KEY_NONE) atomicAdd(&s_np, 1);
    }
    __syncthreads();
    if (tid == 0) s_thr = s_np == k ? s_list[k - 1] : KEY_NONE;
    __syncthreads();
    int par = 0;
    for (int64_t base = k; base < total; base += EXACT_MSTEP, par ^= 1) {
        const uint64_t thr = s_thr;
#pragma unroll
        for (int u = 0; u < EXACT_MSTEP / 256; ++u) {
            const int64_t i = base + u * 256 + tid;
            if (i < total) {
                const uint64_t key = in[i];
                if (key < thr) {  // KEY_NONE never is
                    const int pos = atomicAdd(&s_cnt, 1);
                    s_cand[pos] = key;
                    if (pos + 1 > LIMIT) atomicAdd(&s_flag[par], 1);  // (several lanes may say so in one step)
                }
            }
        }
        __syncthreads();
        if (s_flag[par]) {
            exact_flush(s_list, k, s_cand, &s_cnt, &s_np, &s_cur, &s_thr, tid);
            if (tid == 0) s_flag[par] = 0;
            __syncthreads();
        }
    }
    exact_flush(s_list, k, s_cand, &s_cnt, &s_np, &s_cur, &s_thr, tid);
    __syncthreads();
    const uint64_t* fin = s_list + s_cur * k;
    const int np = s_np;
    for (int j = tid; j < k; j += 256) {
        const size_t o = (size_t)blockIdx.x * k + j;
        if (j < np) {
            const float d = key_dist(fin[j]);
            labels[o] = key_id(fin[j]);
            dist[o] = metric == LM_METRIC_L2 ? d : -d;
        } else {
            labels[o] = -1;
            dist[o] = metric == LM_METRIC_L2 ? __builtin_inff() : -__builtin_inff();
        }
    }
}

template <int NCH, bool L2, bool F16>
static int launch_exact_scan(const void* d_table, int64_t ntable, const float* d_q, int64_t nq, int32_t k, const uint32_t* d_allow, const ExactPlan& p,
                             uint64_t* part, hipStream_t st) {
    constexpr int R = NCH <= 6 ? 2 : 1;
    static DynLdsAttr attr;
    const int qalloc = (int)std::min<int64_t>(EXACT_QT, nq);
    const size_t shmem = (size_t)qalloc * (NCH * 256 + 2 * (size_t)k * 8 + EXACT_CAP * 8);
    LM_HIP(ensure_dyn_lds(attr, (const void*)k_exact_scan<NCH, L2, F16, R>, shmem));
    hipLaunchKernelGGL((k_exact_scan<NCH, L2, F16, R>), dim3((unsigned)(p.S * p.nqt)), dim3(256), shmem, st, d_table, ntable, d_q, nq, (int)k, d_allow,
                       (int)p.S, p.rows, qalloc, part);
    return LM_OK;
}

}  // namespace lm

extern "C" {

size_t lm_exact_search_workspace_bytes(int64_t ntable, int64_t nq, int32_t k) {
    if (ntable < 0 || nq < 0 || k < 1 || k > LM_EXACT_MAX_K) return 0;
    return (size_t)exact_plan(ntable, nq).S * (size_t)nq * (size_t)k * sizeof(uint64_t);
}

int lm_exact_search(const void* d_table, int32_t dtype, int64_t ntable, int32_t d_padded, int32_t metric, const float* d_q, int64_t nq, int32_t k,
                    const uint32_t* d_allow, float* d_distances, int64_t* d_labels, void* d_workspace, size_t workspace_bytes, void* stream) {
    if (d_padded <= 0 || d_padded % 64) LM_FAIL(LM_EINVAL, "d_padded must be a positive multiple of 64");
    switch (d_padded / 64) {
        case 1: case 2: case 3: case 4: case 5: case 6: case 8: case 12: case 16: break;
        default: LM_FAIL(LM_EINVAL, "unsupported padded dimension (supported: 64..384, 512, 768, 1024)");
    }
    if (dtype != LM_DTYPE_F32 && dtype != LM_DTYPE_F16) LM_FAIL(LM_EINVAL, "dtype must be f32 or f16");
    if (metric != LM_METRIC_INNER_PRODUCT && metric != LM_METRIC_L2) LM_FAIL(LM_EINVAL, "unknown metric");
    if (k < 1 || k > LM_EXACT_MAX_K) LM_FAIL(LM_EINVAL, "k must be in [1, LM_EXACT_MAX_K = " + std::to_string(LM_EXACT_MAX_K) + "]");
    if (nq < 0 || ntable < 0) LM_FAIL(LM_EINVAL, "nq / ntable must not be negative");
    if (ntable > 0x7fffffffll) LM_FAIL(LM_EINVAL, "ntable must fit the 31-bit id of the (distance, id) key");
    const ExactPlan p = exact_plan(ntable, nq);
    if (p.S * p.nqt > 0x7fffffffll) LM_FAIL(LM_EINVAL, "nq too large for one launch");
    if (workspace_bytes < lm_exact_search_workspace_bytes(ntable, nq, k)) LM_FAIL(LM_EINVAL, "workspace smaller than lm_exact_search_workspace_bytes");
    if (nq == 0) return LM_OK;
    if (!d_q || !d_distances || !d_labels || !d_workspace || (ntable > 0 && !d_table)) LM_FAIL(LM_EINVAL, "NULL buffer");
    hipStream_t st = (hipStream_t)stream;
    uint64_t* part = (uint64_t*)d_workspace;
    const bool l2 = metric == LM_METRIC_L2, f16 = dtype == LM_DTYPE_F16;
    int rc = LM_OK;
#define GO(nch)                                                                                                          \
    case nch:                                                                                                            \
        if (l2 && f16) rc = launch_exact_scan<nch, true, true>(d_table, ntable, d_q, nq, k, d_allow, p, part, st);       \
        else if (l2) rc = launch_exact_scan<nch, true, false>(d_table, ntable, d_q, nq, k, d_allow, p, part, st);        \
        else if (f16) rc = launch_exact_scan<nch, false, true>(d_table, ntable, d_q, nq, k, d_allow, p, part, st);       \
        else rc = launch_exact_scan<nch, false, false>(d_table, ntable, d_q, nq, k, d_allow, p, part, st);               \
        break
    switch (d_padded / 64) {
        GO(1); GO(2); GO(3); GO(4); GO(5); GO(6); GO(8); GO(12); GO(16);
    }
#undef GO
    if (rc) return rc;
    LM_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_exact_merge, dim3((unsigned)nq), dim3(256), 0, st, (const uint64_t*)part, (int)p.S, (int)k, metric, d_distances, d_labels);
    LM_HIP(hipGetLastError());
    return LM_OK;
}

// queries [n][D] on the device -> the kernel's [n][Dp] (the index's own padding buffer, as lm_index_search_device), workspace grown on demand
static int exact_on_index(lm_index* ix, int64_t n, const float* d_x, int32_t k, const uint32_t* d_allow, float* d_dist, int64_t* d_labels) {
    hipStream_t st = ix->stream;
    const float* d_q = nullptr;
    if (int rc = pad_queries(ix, n, d_x, &d_q)) return rc;
    if (int rc = ix->d_exact_ws.reserve(lm_exact_search_workspace_bytes(ix->N, n, k))) return rc;
    if (int rc = lm_exact_search(ix->d_table, ix->table_dtype, ix->N, ix->Dp, ix->metric, d_q, n, k, d_allow, d_dist, d_labels, ix->d_exact_ws.get(),
                                 ix->d_exact_ws.capacity(), st))
        return rc;
    LM_HIP(hipStreamSynchronize(st));
    return LM_OK;
}

static int exact_index_checks(lm_index* ix, int64_t n, int32_t k) {
    if (!ix) LM_FAIL(LM_EINVAL, "NULL index");
    if (n < 0) LM_FAIL(LM_EINVAL, "n must not be negative");
    if (k < 1 || k > LM_EXACT_MAX_K) LM_FAIL(LM_EINVAL, "k must be in [1, LM_EXACT_MAX_K = " + std::to_string(LM_EXACT_MAX_K) + "]");
    if (!ix->d_table) LM_FAIL(LM_ESTATE, "index stores no embeddings (pruned): the exact search needs an attached table");
    return LM_OK;
}

int lm_index_search_exact_device(lm_index* ix, int64_t n, const float* d_x, int32_t k, const uint32_t* d_allow, float* d_distances,
                                 int64_t* d_labels) {
    if (int rc = exact_index_checks(ix, n, k)) return rc;
    if (n == 0) return LM_OK;
    if (!d_x || !d_distances || !d_labels) LM_FAIL(LM_EINVAL, "NULL buffer");
    LM_HIP(hipSetDevice(ix->device));
    return exact_on_index(ix, n, d_x, k, d_allow, d_distances, d_labels);
}

int lm_index_search_exact(lm_index* ix, int64_t n, const float* x, int32_t k, const uint32_t* allow, float* distances, int64_t* labels) {
    if (int rc = exact_index_checks(ix, n, k)) return rc;
    if (n == 0) return LM_OK;
    if (!x || !distances || !labels) LM_FAIL(LM_EINVAL, "NULL buffer");
    LM_HIP(hipSetDevice(ix->device));
    const uint32_t* d_allow = nullptr;
    if (int rc = upload_allow(ix, allow, &d_allow)) return rc;
    if (int rc = stage_in(ix, x, n, k)) return rc;
    if (int rc = exact_on_index(ix, n, ix->d_stage_x.get(), k, d_allow, ix->d_stage_d.get(), ix->d_stage_l.get())) return rc;
    return stage_out(ix, distances, labels, n, k);
}

}  // extern "C"
