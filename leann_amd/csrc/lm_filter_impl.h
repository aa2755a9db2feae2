// lm_filter_impl.h -- allow-list for the HNSW graph search (lm_index_search_filtered*): k_filter_collect, k_filter_init / _finalize / _total.
// Part of lm_search.hip's translation unit (included there after lm_kernels_misc.h); see its header comment.
//
// faiss filters inside the graph search (HNSW::search_from_candidates with an IDSelector): every evaluated node steers the walk, only selected
// nodes enter the result heap.  Here the walk is lm_index_search's, untouched -- k_expand, k_update and everything they read or write are the
// unfiltered call's -- and the result heap is a second, per-query sorted list res[B][k] in global memory that k_filter_collect feeds once per
// lock-step round, after k_expand (the round's phase and new-list are final) and before k_update (which may end the query).
//
// E, the set the filtered result is the best k of (intersected with the allow-list): the seed the descent hands to level 0 and every node that
// enters a new-list while the query is in its beam phase.  Nodes the upper-level descent evaluates are not in E (faiss's greedy descent pushes
// nothing to the results either).
//
// k_filter_collect  one 256-thread workgroup per query.  Not in its beam phase (or done): return.  First beam round (nres[q] < 0): the seed's key
//                   is pool[0] without the expanded flag -- the pool holds exactly the seed until the first beam-phase k_update merges into it,
//                   and the key is k_update's own, nothing is recomputed.  New-list: the allow bit is tested first (a rejected row is never
//                   loaded), then load_row / row_reduce / make_key exactly as k_update forms its keys (the same bits); keys not below the list's
//                   k-th key are dropped when the list is full; the survivors (an LDS counter hands out their places: the ORDER is not fixed,
//                   the SET is, and the merge ranks by key) are merged by rank_merge_unsorted and the list is written back.
//                   It computes each allowed distance a second time; the rows were fetched by the same round microseconds earlier.
//                   It writes res, nres and nallow only: ndis_q, the pool, visited and every counter the walk reads stay as they are.
// LDS: list[k] | merged list[k] | survivors[next_pow2(maxnew)].
#pragma once

namespace lm {

struct FilterDev {
    const uint32_t* allow;       // NULL = every node, else ceil(N / 32) words (lm_exact_search's layout)
    uint64_t* res;               // B x k sorted keys (expanded flag clear)
    int32_t* nres;               // B: keys in the list; -1 = the query's seed has not been collected yet
    unsigned long long* nallow;  // B: (query, node) pairs that passed the allow test = |E n allowed| per query; [B] = their sum (k_filter_total)
    int32_t k;
};

__global__ void k_filter_init(FilterDev f, int B) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= B) return;
    f.nres[q] = -1;
    f.nallow[q] = 0ull;
}

__device__ __forceinline__ bool filter_allows(const uint32_t* allow, int32_t v) { return allow == nullptr || ((allow[v >> 5] >> (v & 31)) & 1u); }

template <int NCH, bool L2, bool F16>
__global__ __launch_bounds__(256) void k_filter_collect(WsDev ws, UpdateArgs a, FilterDev f) {
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ int s_cnt, s_nall;
    const int q = blockIdx.x;
    const int tid = threadIdx.x;
    if (ws.phase[q] != PH_BEAM) return;  // done, or still descending: the same for every thread
    const int k = f.k;
    const int n = ws.nnew[q];
    uint64_t* res = f.res + (size_t)q * k;
    uint64_t* lres = (uint64_t*)smem;  // k
    uint64_t* out = lres + k;          // k
    uint64_t* newk = out + k;          // up to n <= maxnew survivors
    int np0 = f.nres[q];
    const bool first = np0 < 0;
    bool seed_in = false;
    if (first) {
        // the seed is a member of E whether it has neighbours or not
        const uint64_t seed = ws.pool[(size_t)q * ws.ef] & ~KEY_EXPANDED;
        seed_in = filter_allows(f.allow, key_id(seed));
        np0 = seed_in ? 1 : 0;
        if (seed_in && tid == 0) lres[0] = seed;
    } else {
        for (int i = tid; i < np0; i += 256) lres[i] = res[i];
    }
    if (tid == 0) {
        s_cnt = 0;
        s_nall = 0;
    }
    __syncthreads();
    const uint64_t thr = np0 == k ? lres[k - 1] : KEY_NONE;  // the list is full: only keys below its k-th can enter

    const int lane16 = tid & 15, sg = tid >> 4;
    float4 qv[NCH];
    load_query<NCH>(a.Q, q, lane16, qv);
    const int32_t* newid = ws.newid + (size_t)q * ws.maxnew;
    for (int i = sg; i < n; i += 16) {
        const int32_t v = newid[i];
        if (!filter_allows(f.allow, v)) continue;  // the same for the 16 lanes of a group
        int64_t s = v;  // UpdateArgs' addressing modes, as in k_update
        if (a.by_rank == 1) s = a.identity ? i : ws.word_rank[v >> 5] + __popc(ws.rbm_snap[v >> 5] & ((1u << (v & 31)) - 1u));
        else if (a.by_rank == 2) s = ws.memo_slot[v];
        float4 e[NCH];
        load_row<NCH, F16>(a.E, s, lane16, e);
        const float d = row_reduce<NCH, L2>(e, qv);
        if (lane16 == 0) {
            atomicAdd(&s_nall, 1);
            const uint64_t key = make_key(d, v);
            if (key < thr) newk[atomicAdd(&s_cnt, 1)] = key;
        }
    }
    __syncthreads();
    const int m = s_cnt;  // may exceed k (k = 1, a long new-list), may be 0
    const int np1 = min(k, np0 + m);
    const uint64_t* fin = lres;
    if (m > 0) {
        rank_merge_unsorted<256>(lres, np0, newk, m, out, k, tid);
        fin = out;
    }
    if (first || m > 0)
        for (int i = tid; i < np1; i += 256) res[i] = fin[i];
    if (tid == 0) {
        f.nres[q] = np1;
        f.nallow[q] += (unsigned long long)(s_nall + (seed_in ? 1 : 0));
    }
}

// res -> (labels, distances), as k_finalize decodes the pool
__global__ void k_filter_finalize(FilterDev f, int B, int32_t metric, int64_t* labels, float* dist) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= B * f.k) return;
    const int q = t / f.k, i = t % f.k;
    if (i < f.nres[q]) {
        const uint64_t key = f.res[(size_t)q * f.k + i];
        const float d = key_dist(key);
        labels[t] = key_id(key);
        dist[t] = metric == LM_METRIC_L2 ? d : -d;
    } else {
        labels[t] = -1;
        dist[t] = metric == LM_METRIC_L2 ? __builtin_inff() : -__builtin_inff();
    }
}

// nallow[B] = the sum of the per-query counts (no shared counter in the round kernel)
__global__ __launch_bounds__(256) void k_filter_total(FilterDev f, int B) {
    __shared__ unsigned long long red[4];
    unsigned long long a = 0;
    for (int q = threadIdx.x; q < B; q += 256) a += f.nallow[q];
    for (int m = 32; m >= 1; m >>= 1) a += __shfl_xor(a, m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) f.nallow[B] = red[0] + red[1] + red[2] + red[3];
}

}  // namespace lm
