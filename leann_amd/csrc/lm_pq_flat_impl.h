// lm_pq_flat_impl.h -- flat PQ scan with an allow-list + the PQ path's rerank tail: the filtered search of an index that stores no embeddings
// (it keeps its PQ codes and the recompute provider).  Included at the end of lm_search.hip (shares make_key / rank_merge_unsorted, the
// exact scan's slice / pending-list / merge scheme and lm_pq_impl.h's pq_rerank_tail).  Arithmetic contract: oracle/lm_oracle_pq.c -- the lookup
// table is orc_pq_lut (k_pq_traverse's table arithmetic restated), a row's distance orc_pq_adc, the ranking the (distance, id) key of every
// traversal kernel: labels AND distance bits are a function of the inputs' bits alone.
//
// Reference surface: the reference filters AFTER the graph search (leann/api.py:785-790: metadata_filters), so a filtered query on a pruned
// index returns fewer than top_k hits -- at 1 % selectivity usually none.  A flat scan of the N x m code bytes takes the allow-list for free,
// walks no graph (a filter cannot disconnect it), and its L best allowed rows go through the deferred-fetch exact rerank in one provider call.
//
// k_pq_flat_scan   one 1024-thread workgroup per (row slice, tile of qt queries).  The tile's lookup tables are built in LDS (m KB each); then
//                  every thread takes one row per step: it tests the row's allow bit FIRST (a rejected row is never loaded), requests all
//                  16-byte pieces of the code row together (consecutive threads read consecutive rows: a wave covers 64 m contiguous bytes)
//                  and scores the row against every query of the tile.  Per query the workgroup keeps a sorted top-L key list in LDS and
//                  its L-th key as the threshold: a key that is not below it costs one comparison.  Survivors go to a per-query pending list
//                  (PQF_CAP = 1280 keys; an LDS integer counter hands out the places -- the ORDER inside the pending list is not fixed, the
//                  SET is, and the merge ranks by key); when a pending list could overflow in the next step the workgroup merges it into
//                  the list (rank_merge_unsorted).  The "merge now" flag alternates between two words, as in k_exact_scan.  The slice's list
//                  goes to the workspace: part[(query * S + slice) * L + j], KEY_NONE = empty.
// k_pq_flat_merge  one 256-thread workgroup per query: the S sorted partial lists stream past the same threshold / pending list / merge,
//                  seeded with slice 0's list; writes the caller's labels and distances (stand-alone form) or ws.pool / ws.npool (index form).
// k_pq_flat_count  the index form's totals: ndis = allowed rows x queries, nrounds = 1.
// No float atomics, nothing depends on which workgroup finishes first.
//
// Slicing policy -- a pure function of (ntotal, nq, m, L): pq_flat_plan().
//     per_q = 1024 m + 16 L + 8 PQF_CAP               bytes of LDS per query: table, the list and the list being merged into, pending keys
//     qt    = min(8, floor(PQF_LDS / per_q))           queries per tile; 0 = the state does not fit (LM_EINVAL).  PQF_LDS = 158 KB
//     nqt   = max(1, ceil(nq / qt))                    query tiles
//     s0    = clamp(ceil(ntotal / 2048), 1, max(1, 512 / nqt))
//     rows  = max(32, ceil(ntotal / s0) rounded up to a multiple of 32)      rows per slice
//     S     = max(1, ceil(ntotal / rows))              slices; the last one holds ntotal - (S - 1) rows
// One query: ntotal <= 2048 is one slice, 2049 .. 4096 two, 4097 three, 20 000 ten (nine of 2016 rows and a last one of 1856), 1M rows 489 of
// 2048.  qt is one at m = 96, two at m = 48, eight at m = 8 and L <= 112.  Merge: 2 x 1024 x 8 + 1024 x 8 = 24 KB of LDS.
#pragma once

namespace lm {

constexpr int PQF_NTH = 1024;            // threads of the scan = rows per step
constexpr int PQF_QT = 8;                // most queries per tile
constexpr int PQF_SLICE_ROWS = 2048;     // no slice is cut smaller than this (except the last)
constexpr int PQF_TARGET_WG = 512;       // slices x query tiles the policy aims for
constexpr int PQF_CAP = PQF_NTH + 256;   // scan: pending keys per query (a step appends at most PQF_NTH)
constexpr int PQF_LDS = 158 * 1024;      // dynamic LDS of the scan: 160 KB minus the kernel's static words
constexpr int PQF_MAX_M = 160;           // > PQF_LDS / 1024: sub-quantisers whose table can fit at all
constexpr int PQF_MCAP = 1024;           // merge: pending keys
constexpr int PQF_MSTEP = 512;           // merge: keys read per step

struct PqFlatPlan {
    int64_t qt, nqt, S, rows;
};
static PqFlatPlan pq_flat_plan(int64_t ntotal, int64_t nq, int32_t m, int32_t L) {
    PqFlatPlan p;
    const int64_t per_q = (int64_t)1024 * m + (int64_t)16 * L + 8 * PQF_CAP;
    p.qt = std::min<int64_t>(PQF_QT, PQF_LDS / per_q);
    p.nqt = p.qt > 0 ? std::max<int64_t>(1, (nq + p.qt - 1) / p.qt) : 1;
    const int64_t smax = std::max<int64_t>(1, PQF_TARGET_WG / p.nqt);
    const int64_t s0 = std::min(smax, std::max<int64_t>(1, (ntotal + PQF_SLICE_ROWS - 1) / PQF_SLICE_ROWS));
    p.rows = std::max<int64_t>(32, ((ntotal + s0 - 1) / s0 + 31) / 32 * 32);
    p.S = std::max<int64_t>(1, (ntotal + p.rows - 1) / p.rows);
    return p;
}

struct PqFlatOff {
    int32_t v[PQF_MAX_M + 1];  // chunk offsets, by value: the stand-alone form has them on the host only
};

struct PqFlatArgs {
    const uint8_t* codes;    // ntotal x m
    const float* codebooks;  // chunk j: 256 centroids x len_j floats at 256 * off[j]
    const float* Q;          // nq x ldq
    const uint32_t* allow;   // NULL = every row
    uint64_t* part;          // nq x S x L
    int64_t ntotal, nq, rows_per_slice;
    int32_t m, metric, ldq, L, S, qt;
};

// exact_flush (lm_exact_impl.h) for a workgroup of NT threads: pending keys cand[0 .. *cnt) into the sorted list (two buffers of k keys at `lists`,
// *cur names the live one).  Every thread calls it between two barriers that no thread has passed while *cnt could still change; ends with a
// barrier when it had work, thread 0's updates of the four words become visible at the caller's next barrier.
template <int NT>
__device__ __forceinline__ void pqf_flush(uint64_t* lists, int k, const uint64_t* cand, int* cnt, int* np, int* cur, uint64_t* thr, int tid) {
    const int n = *cnt, np0 = *np, c = *cur;
    if (n == 0) return;  // the same for every thread
    uint64_t* dst = lists + (c ^ 1) * k;
    rank_merge_unsorted<NT>(lists + c * k, np0, cand, n, dst, k, tid);
    if (tid == 0) {
        const int np1 = min(k, np0 + n);
        *np = np1;
        *cnt = 0;
        *cur = c ^ 1;
        *thr = np1 == k ? dst[k - 1] : KEY_NONE;
    }
}

// NP > 0: m = 16 NP and the code rows are 16-byte aligned -- a row is NP 16-byte pieces, all requested before the first lookup, and kept in registers
// for every query of the tile.  NP = 0: any m (a multiple of 4), dwords.
template <int NP>
__global__ __launch_bounds__(PQF_NTH) void k_pq_flat_scan(PqFlatArgs a, PqFlatOff off) {
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ int32_t s_off[PQF_MAX_M + 1];
    __shared__ int s_cnt[PQF_QT], s_np[PQF_QT], s_cur[PQF_QT], s_flag[2];
    __shared__ uint64_t s_thr[PQF_QT];
    constexpr int LIMIT = PQF_CAP - PQF_NTH;  // a step appends at most PQF_NTH keys per query
    typedef unsigned pqf_u32x4 __attribute__((ext_vector_type(4)));
    const int tid = threadIdx.x, m = a.m, L = a.L, S = a.S;
    const int s = (int)(blockIdx.x % (unsigned)S);
    const int64_t q0 = (int64_t)(blockIdx.x / (unsigned)S) * a.qt;
    const int nqh = (int)min((int64_t)a.qt, a.nq - q0);
    const int ne = m * 256;
    float* lut = (float*)smem;                              // qt x m x 256
    uint64_t* lists = (uint64_t*)(lut + (size_t)a.qt * ne);  // qt x 2 x L
    uint64_t* cand = lists + (size_t)a.qt * 2 * L;          // qt x PQF_CAP
    if (tid <= m) s_off[tid] = off.v[tid];
    if (tid < PQF_QT) {
        s_cnt[tid] = 0;
        s_np[tid] = 0;
        s_cur[tid] = 0;
        s_thr[tid] = KEY_NONE;
    }
    if (tid < 2) s_flag[tid] = 0;
    __syncthreads();
    // ---- lookup tables: k_pq_traverse's arithmetic (orc_pq_lut): sequential fmaf over the chunk's dimensions, negated for inner product; the loads of
    //      four entries (4-element chunks) or of four elements are requested before the first is used, the fmaf chain keeps its order ----
    const bool l2 = a.metric == LM_METRIC_L2;
    for (int q = 0; q < nqh; ++q) {
        const float* qv = a.Q + (size_t)(q0 + q) * a.ldq;
        float* lq = lut + (size_t)q * ne;
        constexpr int EU = 4;
        for (int e0 = tid; e0 < ne; e0 += EU * PQF_NTH) {
            int lov[EU], lenv[EU];
            bool four = true;
#pragma unroll
            for (int u = 0; u < EU; ++u) {
                const int e = min(e0 + u * PQF_NTH, ne - 1);  // (clamped: the tail group recomputes the last entry, stores are guarded)
                lov[u] = s_off[e >> 8];
                lenv[u] = s_off[(e >> 8) + 1] - lov[u];
                four = four && lenv[u] == 4;
            }
            if (four) {
                float qe[EU][4], ce[EU][4];
#pragma unroll
                for (int u = 0; u < EU; ++u) {
                    const int e = min(e0 + u * PQF_NTH, ne - 1);
                    const float* cb = a.codebooks + (size_t)256 * lov[u] + (size_t)(e & 255) * 4;
                    const float* qs = qv + lov[u];
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        qe[u][t] = qs[t];
                        ce[u][t] = cb[t];
                    }
                }
#pragma unroll
                for (int u = 0; u < EU; ++u) {
                    float acc = 0.0f;
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        if (l2) {
                            const float d = qe[u][t] - ce[u][t];
                            acc = __builtin_fmaf(d, d, acc);
                        } else {
                            acc = __builtin_fmaf(qe[u][t], ce[u][t], acc);
                        }
                    }
                    if (e0 + u * PQF_NTH < ne) lq[e0 + u * PQF_NTH] = l2 ? acc : -acc;
                }
            } else {
#pragma unroll
                for (int u = 0; u < EU; ++u) {
                    const int e = e0 + u * PQF_NTH;
                    if (e < ne) {
                        const float* cb = a.codebooks + (size_t)256 * lov[u] + (size_t)(e & 255) * lenv[u];
                        const float* qs = qv + lov[u];
                        float acc = 0.0f;
                        for (int t = 0; t < lenv[u]; ++t) {
                            if (l2) {
                                const float d = qs[t] - cb[t];
                                acc = __builtin_fmaf(d, d, acc);
                            } else {
                                acc = __builtin_fmaf(qs[t], cb[t], acc);
                            }
                        }
                        lq[e] = l2 ? acc : -acc;
                    }
                }
            }
        }
    }
    __syncthreads();
    // one code dword = sub-quantisers 4 i .. 4 i + 3: one addition to each of the four partial sums (orc_pq_adc's order)
    auto word = [](const float* lq, float& p0, float& p1, float& p2, float& p3, int i, uint32_t w) {
        const float* l4 = lq + ((4 * i) << 8);
        p0 = p0 + l4[w & 255u];
        p1 = p1 + l4[256 + ((w >> 8) & 255u)];
        p2 = p2 + l4[512 + ((w >> 16) & 255u)];
        p3 = p3 + l4[768 + (w >> 24)];
    };
    const int64_t lo = (int64_t)s * a.rows_per_slice, hi = min(a.ntotal, lo + a.rows_per_slice);
    const int mw = m >> 2;
    int par = 0;
    for (int64_t base = lo; base < hi; base += PQF_NTH, par ^= 1) {
        const int64_t row = base + tid;
        const bool valid = row < hi && (a.allow == nullptr || ((a.allow[row >> 5] >> (row & 31)) & 1u));  // the allow word first
        if (valid) {
            pqf_u32x4 c[NP > 0 ? NP : 1];
            const uint32_t* cw = (const uint32_t*)(a.codes + (size_t)row * m);
            if (NP > 0) {
                const pqf_u32x4* c4 = (const pqf_u32x4*)cw;
#pragma unroll
                for (int i = 0; i < NP; ++i) c[i] = c4[i];
            }
            for (int q = 0; q < nqh; ++q) {
                const float* lq = lut + (size_t)q * ne;
                float p0 = 0.0f, p1 = 0.0f, p2 = 0.0f, p3 = 0.0f;
                if (NP > 0) {
#pragma unroll
                    for (int i = 0; i < NP; ++i) {
                        word(lq, p0, p1, p2, p3, 4 * i, c[i][0]);
                        word(lq, p0, p1, p2, p3, 4 * i + 1, c[i][1]);
                        word(lq, p0, p1, p2, p3, 4 * i + 2, c[i][2]);
                        word(lq, p0, p1, p2, p3, 4 * i + 3, c[i][3]);
                    }
                } else {
                    for (int i = 0; i < mw; ++i) word(lq, p0, p1, p2, p3, i, cw[i]);
                }
                const uint64_t key = make_key((p0 + p1) + (p2 + p3), (int32_t)row);
                if (key < s_thr[q]) {  // rejected against the L-th key before any insertion work
                    const int pos = atomicAdd(&s_cnt[q], 1);
                    cand[q * PQF_CAP + pos] = key;
                    if (pos + 1 > LIMIT) atomicAdd(&s_flag[par], 1);  // (several lanes may say so in one step)
                }
            }
        }
        __syncthreads();
        if (s_flag[par]) {  // written in this step only, read after its barrier: the same for every thread
            for (int q = 0; q < nqh; ++q)
                pqf_flush<PQF_NTH>(lists + (size_t)q * 2 * L, L, cand + q * PQF_CAP, &s_cnt[q], &s_np[q], &s_cur[q], &s_thr[q], tid);
            if (tid == 0) s_flag[par] = 0;
            __syncthreads();
        }
    }
    for (int q = 0; q < nqh; ++q)
        pqf_flush<PQF_NTH>(lists + (size_t)q * 2 * L, L, cand + q * PQF_CAP, &s_cnt[q], &s_np[q], &s_cur[q], &s_thr[q], tid);
    __syncthreads();
    for (int q = 0; q < nqh; ++q) {
        const uint64_t* src = lists + (size_t)q * 2 * L + s_cur[q] * L;
        uint64_t* dst = a.part + ((size_t)(q0 + q) * S + s) * L;
        const int np = s_np[q];
        for (int j = tid; j < L; j += PQF_NTH) dst[j] = j < np ? src[j] : KEY_NONE;
    }
}

// labels != NULL: the stand-alone form's outputs [nq][L]; else the index form: pool[q * ef + j] and npool[q]
__global__ __launch_bounds__(256) void k_pq_flat_merge(const uint64_t* part, int S, int L, int metric, float* dist, int64_t* labels, uint64_t* pool,
                                                       int32_t* npool, int ef) {
    __shared__ uint64_t s_list[2 * LM_PQ_FLAT_MAX_L];
    __shared__ uint64_t s_cand[PQF_MCAP];
    __shared__ int s_cnt, s_np, s_cur, s_flag[2];
    __shared__ uint64_t s_thr;
    constexpr int LIMIT = PQF_MCAP - PQF_MSTEP;
    const int tid = threadIdx.x;
    const uint64_t* in = part + (size_t)blockIdx.x * S * L;
    const int64_t total = (int64_t)S * L;
    if (tid == 0) {
        s_cnt = 0;
        s_np = 0;
        s_cur = 0;
        s_flag[0] = s_flag[1] = 0;
    }
    __syncthreads();
    for (int j = tid; j < L; j += 256) {  // slice 0's list seeds the result: sorted, its empty places at the end
        const uint64_t key = in[j];
        s_list[j] = key;
        if (key != KEY_NONE) atomicAdd(&s_np, 1);
    }
    __syncthreads();
    if (tid == 0) s_thr = s_np == L ? s_list[L - 1] : KEY_NONE;
    __syncthreads();
    int par = 0;
    for (int64_t base = L; base < total; base += PQF_MSTEP, par ^= 1) {
        const uint64_t thr = s_thr;
#pragma unroll
        for (int u = 0; u < PQF_MSTEP / 256; ++u) {
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
            pqf_flush<256>(s_list, L, s_cand, &s_cnt, &s_np, &s_cur, &s_thr, tid);
            if (tid == 0) s_flag[par] = 0;
            __syncthreads();
        }
    }
    pqf_flush<256>(s_list, L, s_cand, &s_cnt, &s_np, &s_cur, &s_thr, tid);
    __syncthreads();
    const uint64_t* fin = s_list + s_cur * L;
    const int np = s_np;
    if (labels == nullptr) {
        for (int j = tid; j < np; j += 256) pool[(size_t)blockIdx.x * ef + j] = fin[j];
        if (tid == 0) npool[blockIdx.x] = np;
        return;
    }
    for (int j = tid; j < L; j += 256) {
        const size_t o = (size_t)blockIdx.x * L + j;
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

// the index form's totals (one workgroup): ndis = participating rows x queries, nrounds = 1 (nexpand stays 0)
__global__ __launch_bounds__(256) void k_pq_flat_count(const uint32_t* allow, int64_t ntotal, int64_t nq, unsigned long long* counters) {
    __shared__ unsigned long long red[4];
    unsigned long long x = 0;
    const int64_t nw = (ntotal + 31) / 32;
    if (allow) {
        for (int64_t w = threadIdx.x; w < nw; w += 256) {
            uint32_t v = allow[w];
            if (w == nw - 1 && (ntotal & 31)) v &= (1u << (ntotal & 31)) - 1u;
            x += (unsigned long long)__popc(v);
        }
    } else if (threadIdx.x == 0) {
        x = (unsigned long long)ntotal;
    }
    for (int mk = 32; mk >= 1; mk >>= 1) x += __shfl_xor(x, mk);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    if (threadIdx.x == 0) {
        counters[C_NDIS] = (red[0] + red[1] + red[2] + red[3]) * (unsigned long long)nq;
        counters[C_ROUNDS] = 1ull;
    }
}

template <int NP>
static int launch_pq_flat_scan(const PqFlatArgs& a, const PqFlatOff& off, const PqFlatPlan& p, hipStream_t st) {
    static DynLdsAttr attr;
    const size_t shmem = (size_t)a.qt * ((size_t)1024 * a.m + (size_t)16 * a.L + 8 * PQF_CAP);
    LM_HIP(ensure_dyn_lds(attr, (const void*)k_pq_flat_scan<NP>, shmem));
    hipLaunchKernelGGL((k_pq_flat_scan<NP>), dim3((unsigned)(p.S * p.nqt)), dim3(PQF_NTH), shmem, st, a, off);
    LM_HIP(hipGetLastError());
    return LM_OK;
}

// everything lm_pq_scan rejects; fills `off` (uniform offsets when chunk_offsets is NULL) and the plan
static int pq_flat_validate(int64_t ntotal, int32_t m, const int32_t* chunk_offsets, int32_t d, int32_t metric, int64_t nq, int32_t ldq, int32_t L,
                            PqFlatOff& off, PqFlatPlan& p) {
    if (m < 1 || m % 4 || m > 4096) LM_FAIL(LM_EINVAL, "m must be a positive multiple of 4 (pad the codes with empty chunks), at most 4096");
    if (d < 0) LM_FAIL(LM_EINVAL, "d must not be negative");
    if (chunk_offsets) {
        if (chunk_offsets[0] != 0) LM_FAIL(LM_EINVAL, "chunk_offsets[0] must be 0");
        for (int j = 0; j < m; ++j)
            if (chunk_offsets[j + 1] < chunk_offsets[j]) LM_FAIL(LM_EINVAL, "chunk_offsets must not decrease");
        if (chunk_offsets[m] > d) LM_FAIL(LM_EINVAL, "chunk_offsets[m] exceeds d");
    } else if (d % m) {
        LM_FAIL(LM_EINVAL, "uniform layout: m must divide d");
    }
    if (ldq < d) LM_FAIL(LM_EINVAL, "ldq must be at least d");
    if (L < 1 || L > LM_PQ_FLAT_MAX_L) LM_FAIL(LM_EINVAL, "L must be in [1, LM_PQ_FLAT_MAX_L = " + std::to_string(LM_PQ_FLAT_MAX_L) + "]");
    if (metric != LM_METRIC_INNER_PRODUCT && metric != LM_METRIC_L2) LM_FAIL(LM_EINVAL, "unknown metric");
    if (nq < 0 || ntotal < 0) LM_FAIL(LM_EINVAL, "nq / ntotal must not be negative");
    if (ntotal > 0x7fffffffll) LM_FAIL(LM_EINVAL, "ntotal must fit the 31-bit id of the (distance, id) key");
    p = pq_flat_plan(ntotal, nq, m, L);
    if (p.qt < 1 || m > PQF_MAX_M) LM_FAIL(LM_EINVAL, "PQ scan state (lookup table + lists) does not fit the 160 KB LDS (reduce m or L)");
    if (p.S * p.nqt > 0x7fffffffll) LM_FAIL(LM_EINVAL, "nq too large for one launch");
    for (int j = 0; j <= m; ++j) off.v[j] = chunk_offsets ? chunk_offsets[j] : j * (d / m);
    return LM_OK;
}

// the two launches; `a` carries everything but the plan
static int pq_flat_launch(PqFlatArgs a, const PqFlatOff& off, const PqFlatPlan& p, float* d_dist, int64_t* d_labels, uint64_t* pool, int32_t* npool,
                          int ef, hipStream_t st) {
    a.S = (int32_t)p.S;
    a.qt = (int32_t)p.qt;
    a.rows_per_slice = p.rows;
    const bool pieces = ((uintptr_t)a.codes & 15) == 0;
    int rc = LM_OK;
    switch (pieces ? a.m : 0) {
        case 16: rc = launch_pq_flat_scan<1>(a, off, p, st); break;
        case 32: rc = launch_pq_flat_scan<2>(a, off, p, st); break;
        case 48: rc = launch_pq_flat_scan<3>(a, off, p, st); break;
        case 64: rc = launch_pq_flat_scan<4>(a, off, p, st); break;
        case 96: rc = launch_pq_flat_scan<6>(a, off, p, st); break;
        case 128: rc = launch_pq_flat_scan<8>(a, off, p, st); break;
        default: rc = launch_pq_flat_scan<0>(a, off, p, st); break;
    }
    if (rc) return rc;
    hipLaunchKernelGGL(k_pq_flat_merge, dim3((unsigned)a.nq), dim3(256), 0, st, (const uint64_t*)a.part, (int)p.S, (int)a.L, (int)a.metric, d_dist, d_labels,
                       pool, npool, ef);
    LM_HIP(hipGetLastError());
    return LM_OK;
}

}  // namespace lm

extern "C" {

size_t lm_pq_scan_workspace_bytes(int64_t ntotal, int64_t nq, int32_t m, int32_t L) {
    if (ntotal < 0 || nq < 0 || m < 1 || m % 4 || m > PQF_MAX_M || L < 1 || L > LM_PQ_FLAT_MAX_L) return 0;
    const PqFlatPlan p = pq_flat_plan(ntotal, nq, m, L);
    if (p.qt < 1) return 0;
    return (size_t)p.S * (size_t)nq * (size_t)L * sizeof(uint64_t);
}

int lm_pq_scan(const uint8_t* d_codes, int64_t ntotal, int32_t m, const int32_t* chunk_offsets, const float* d_codebooks, int32_t d, int32_t metric,
               const float* d_q, int64_t nq, int32_t ldq, int32_t L, const uint32_t* d_allow, float* d_distances, int64_t* d_labels, void* d_workspace,
               size_t workspace_bytes, void* stream) {
    PqFlatOff off;
    PqFlatPlan p;
    if (int rc = pq_flat_validate(ntotal, m, chunk_offsets, d, metric, nq, ldq, L, off, p)) return rc;
    if (workspace_bytes < lm_pq_scan_workspace_bytes(ntotal, nq, m, L)) LM_FAIL(LM_EINVAL, "workspace smaller than lm_pq_scan_workspace_bytes");
    if (((uintptr_t)d_codes & 3) != 0) LM_FAIL(LM_EINVAL, "d_codes must be 4-byte aligned (the code rows are read as dwords)");
    if (nq == 0) return LM_OK;
    if (!d_q || !d_distances || !d_labels || !d_workspace || !d_codebooks || (ntotal > 0 && !d_codes)) LM_FAIL(LM_EINVAL, "NULL buffer");
    PqFlatArgs a{};
    a.codes = d_codes; a.codebooks = d_codebooks; a.Q = d_q; a.allow = d_allow; a.part = (uint64_t*)d_workspace;
    a.ntotal = ntotal; a.nq = nq; a.m = m; a.metric = metric; a.ldq = ldq; a.L = L;
    return pq_flat_launch(a, off, p, d_distances, d_labels, nullptr, nullptr, 0, (hipStream_t)stream);
}

// queries [n][D] on the device; everything on the index's stream
static int pq_flat_device(lm_index* ix, int64_t n, const float* d_x, int32_t k, const lm_pq_search_params* params, const uint32_t* d_allow,
                          int64_t* d_labels, float* d_dist) {
    hipStream_t st = ix->stream;
    const lm_pq_search_params& prm = *params;
    const int32_t L = std::max(prm.complexity, k);
    ix->stats = lm_search_stats{};
    if (n == 0) return LM_OK;
    if (ix->N == 0) {
        hipLaunchKernelGGL(k_fill_empty, dim3((unsigned)((n * k + 255) / 256)), dim3(256), 0, st, n * (int64_t)k, ix->metric, d_labels, d_dist);
        LM_HIP(hipStreamSynchronize(st));
        return LM_OK;
    }
    const float* d_q = nullptr;
    if (int rc = pad_queries(ix, n, d_x, &d_q)) return rc;
    const bool rerank = !prm.skip_search_reorder && ((prm.use_deferred_fetch && ix->provider) || ix->d_table != nullptr);
    const int64_t nwbytes = ((ix->N + 31) / 32) * 4;
    const int64_t maxb = std::max<int64_t>(1, std::min<int64_t>(4096, (8ll << 30) / std::max<int64_t>(nwbytes, 1)));  // passes as pq_search_device cuts them
    for (int64_t o = 0; o < n; o += maxb) {
        const int32_t B = (int32_t)std::min<int64_t>(maxb, n - o);
        PqFlatOff off;
        PqFlatPlan p;
        if (int rc = pq_flat_validate(ix->N, ix->pq_m, ix->h_pq_chunk_off.data(), ix->D, ix->metric, B, ix->Dp, L, off, p)) return rc;
        if (int rc = ensure_ws(ix, B, L, 1)) return rc;
        if (int rc = ix->d_pqflat_ws.reserve(lm_pq_scan_workspace_bytes(ix->N, B, ix->pq_m, L))) return rc;
        WsDev& ws = ix->ws;
        LM_HIP(hipMemsetAsync(ws.counters, 0, C_NCOUNTERS * sizeof(unsigned long long), st));
        PqFlatArgs a{};
        a.codes = ix->d_pq_codes.get(); a.codebooks = ix->d_pq_codebooks.get(); a.Q = d_q + (size_t)o * ix->Dp; a.allow = d_allow;
        a.part = (uint64_t*)ix->d_pqflat_ws.get();
        a.ntotal = ix->N; a.nq = B; a.m = ix->pq_m; a.metric = ix->metric; a.ldq = ix->Dp; a.L = L;
        {
            EvScope es(ix, &ix->ev_update);
            if (int rc = pq_flat_launch(a, off, p, nullptr, nullptr, ws.pool, ws.npool, ws.ef, st)) return rc;
        }
        ix->stats.update_launches++;
        hipLaunchKernelGGL(k_pq_flat_count, dim3(1), dim3(256), 0, st, d_allow, ix->N, (int64_t)B, ws.counters);
        if (int rc = pq_rerank_tail(ix, B, a.Q, k, prm, rerank, L, d_dist + (size_t)o * k, d_labels + (size_t)o * k)) return rc;
    }
    LM_HIP(hipStreamSynchronize(st));
    if (ix->profiling) {
        ix->stats.update_ms = drain_events(ix, ix->ev_update);
        ix->stats.provider_ms = drain_events(ix, ix->ev_provider);
    }
    return LM_OK;
}

static int pq_flat_index_checks(lm_index* ix, int64_t n, int32_t k, const lm_pq_search_params* params) {
    LM_NOT_ON_VIEW(ix, "lm_pq_flat_search");
    if (!ix || !params || n < 0 || k <= 0) LM_FAIL(LM_EINVAL, "bad search arguments");
    if (params->complexity <= 0) LM_FAIL(LM_EINVAL, "complexity must be positive");
    if (params->recompute_neighbors) LM_FAIL(LM_EINVAL, "recompute_neighbors != 0 is not supported (as in lm_pq_batch_search)");
    if (std::max(params->complexity, k) > LM_PQ_FLAT_MAX_L)
        LM_FAIL(LM_EINVAL, "max(complexity, k) must be at most LM_PQ_FLAT_MAX_L = " + std::to_string(LM_PQ_FLAT_MAX_L));
    if (!ix->d_pq_codes.get()) LM_FAIL(LM_ESTATE, "no PQ codes attached (lm_pq_attach)");
    if (params->use_deferred_fetch && !ix->provider && !ix->d_table)
        LM_FAIL(LM_ESTATE, "deferred fetch requested but neither an embedding provider nor stored embeddings are attached");
    PqFlatOff off;  // the scan's own envelope (table + lists in the LDS), here so that nothing is staged or launched before it is known to hold
    PqFlatPlan p;
    return pq_flat_validate(ix->N, ix->pq_m, ix->h_pq_chunk_off.data(), ix->D, ix->metric, std::min<int64_t>(n, 4096), ix->Dp, std::max(params->complexity, k),
                            off, p);
}

int lm_pq_flat_search_device(lm_index* ix, int64_t n, const float* d_x, int32_t k, const lm_pq_search_params* params, const uint32_t* d_allow,
                             int64_t* d_labels, float* d_distances) {
    if (int rc = pq_flat_index_checks(ix, n, k, params)) return rc;
    if (n > 0 && (!d_x || !d_labels || !d_distances)) LM_FAIL(LM_EINVAL, "NULL buffer");
    LM_HIP(hipSetDevice(ix->device));
    return pq_flat_device(ix, n, d_x, k, params, d_allow, d_labels, d_distances);
}

int lm_pq_flat_search(lm_index* ix, int64_t n, const float* x, int32_t k, const lm_pq_search_params* params, const uint32_t* allow, int64_t* labels,
                      float* distances) {
    if (int rc = pq_flat_index_checks(ix, n, k, params)) return rc;
    if (n > 0 && (!x || !labels || !distances)) LM_FAIL(LM_EINVAL, "NULL buffer");
    LM_HIP(hipSetDevice(ix->device));
    if (n == 0) {
        ix->stats = lm_search_stats{};
        return LM_OK;
    }
    const uint32_t* d_allow = nullptr;  // (an empty index: no word to upload, and pq_flat_device launches nothing that reads the list)
    if (int rc = upload_allow(ix, allow, &d_allow)) return rc;
    if (int rc = stage_in(ix, x, n, k)) return rc;
    if (int rc = pq_flat_device(ix, n, ix->d_stage_x.get(), k, params, d_allow, ix->d_stage_l.get(), ix->d_stage_d.get())) return rc;
    return stage_out(ix, distances, labels, n, k);
}

}  // extern "C"
