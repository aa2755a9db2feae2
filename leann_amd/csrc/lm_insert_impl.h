// lm_insert_impl.h -- index build time: one insert step of the batched HNSW builder as ONE library call on a view index
// (lm_graph_insert_batch): gather the batch's table rows as queries, search the level as it stands (the view's own search), form every
// row's candidate list (the search result; in refinement merged with the row's current links, the node itself dropped, deduped by id,
// re-ordered by distance), select neighbours, turn the keep mask into forward and reverse edges, clear the refined rows, and hand the
// edges -- ONCE -- to the link insertion.  Included at the end of lm_search.hip after lm_link_impl.h and lm_prune_impl.h (link_launch and
// select_launch are lm_graph_add_links' and lm_select_neighbors' launches, their kernels unchanged; do_search_device is the view's
// search); include/leann_mi355x.h states the contract, tests/insert_ref/lm_insert_ref.c restates it.
//
// Reference surface replaced: index.add of leann_backend_hnsw/hnsw_backend.py:66-94 (faiss searches, selects and links inside that one
// call), leann_amd/gpu_graph_build.py's torch form of the glue between the kernels (build_graph_gpu's insert(): gather, sign flips,
// cat, two argsorts + gather + scatter_ for the dedupe, a third argsort, boolean-mask indexing for the edge lists -- a host
// synchronisation each --, cat, index_put for the clearing, and inserted.sum() once per batch).
//
// Shape: everything is enqueued on the index's stream; the only host synchronisation is the view search's own counter read.
//   k_insert_queries  one lane per query element: the table row of batch[i], fp16 widened, zeros for a void row (id outside [0, n));
//   (the view search) lm_index_search_device's body on those queries;
//   k_insert_merge    one wave per row (LINK_NT: wave-level barriers only).  The K <= LM_SELECT_MAX_K entries live in LDS: id, distance
//                     bits as they came, and one 64-bit key.  replace == 0: labels and distances are converted and the non-finite ones
//                     blanked, nothing moves.  replace == 1: a bitonic sort by (id, position) puts equal ids side by side, first
//                     occurrence first, so that a repeat is an entry whose left neighbour has its id; a second one by (distance bits made
//                     order preserving, -0 folded; position) is the stable order of the survivors, empties last;
//   select_launch     k_select_neighbors on (cand, cdist);
//   k_insert_edges    one wave per row: the rank of a kept slot = kept slots in the 64-slot pieces before it + popcount of the piece's
//                     ballot below its lane.  Writes all 2 m edge slots of the row (the invalid ones too) and, in refinement, clears row v;
//   link_launch       lm_graph_add_links' four kernels on the 2 b m edges.
#pragma once

namespace lm {

// (on the bits: the answer must not depend on what the compiler is allowed to assume about floating-point values)
__device__ __forceinline__ bool insert_finite(float d) { return (__builtin_bit_cast(uint32_t, d) & 0x7f800000u) != 0x7f800000u; }

__global__ __launch_bounds__(256) void k_insert_queries(const void* table, int f16, int64_t n, int D, int Dp, const int32_t* batch, int64_t b, float* q) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= b * D) return;
    const int64_t i = t / D;
    const int c = (int)(t % D);
    const int32_t v = batch[i];
    float x = 0.0f;
    if (v >= 0 && (int64_t)v < n) x = f16 ? __half2float(((const __half*)table)[(int64_t)v * Dp + c]) : ((const float*)table)[(int64_t)v * Dp + c];
    q[t] = x;
}

// One wave per batch row.  s_id / s_d: the entries in concatenation order (search result, then the row's slots); s_key: the sort keys.
__global__ __launch_bounds__(LINK_NT) void k_insert_merge(const int64_t* labels, const float* sdist, int l2, const int32_t* batch, int64_t n, int kk, int replace,
                                                          int cap, const int32_t* adj, const float* dist, int32_t* cand, float* cdist) {
    __shared__ uint64_t s_key[LM_SELECT_MAX_K];
    __shared__ int32_t s_id[LM_SELECT_MAX_K];
    __shared__ float s_d[LM_SELECT_MAX_K];
    const int tid = threadIdx.x;
    const int64_t i = blockIdx.x;
    const int32_t v = batch[i];
    const bool live = v >= 0 && (int64_t)v < n;  // a void row: every entry empty, nothing dereferenced
    const int K = kk + (replace ? cap : 0);
    int32_t* oc = cand + i * K;
    float* od = cdist + i * K;
    for (int p = tid; p < K; p += LINK_NT) {
        int32_t id = -1;
        float d = __builtin_inff();
        if (live && p < kk) {
            const int64_t lab = labels[i * kk + p];
            if (lab >= 0 && lab < n && !(replace && lab == (int64_t)v)) {
                id = (int32_t)lab;
                const float s = sdist[i * kk + p];
                d = l2 ? s : -s;  // what the search decoded, negated back: exact
            }
        } else if (live) {
            const int32_t u = adj[(int64_t)v * cap + (p - kk)];
            if (u >= 0 && (int64_t)u < n) {
                id = u;
                d = dist[(int64_t)v * cap + (p - kk)];
            }
        }
        s_id[p] = id;
        s_d[p] = d;
    }
    __syncthreads();
    if (!replace) {
        for (int p = tid; p < K; p += LINK_NT) {
            const float d = s_d[p];
            const bool ok = s_id[p] >= 0 && insert_finite(d);
            oc[p] = ok ? s_id[p] : -1;
            od[p] = ok ? d : __builtin_inff();
        }
        return;
    }
    int P = 1;
    while (P < K) P <<= 1;
    // ---- repeats: equal ids side by side, the earliest position first
    for (int p = tid; p < P; p += LINK_NT) s_key[p] = (p < K && s_id[p] >= 0) ? (((uint64_t)(uint32_t)s_id[p] << 32) | (uint64_t)(uint32_t)p) : KEY_NONE;
    __syncthreads();
    sort_keys<LINK_NT>(s_key, P, tid);
    for (int j = tid; j < P; j += LINK_NT) {
        const uint64_t key = s_key[j];
        if (j > 0 && key != KEY_NONE && (uint32_t)(key >> 32) == (uint32_t)(s_key[j - 1] >> 32)) s_id[(uint32_t)key] = -1;  // (positions are distinct: no two lanes write one word)
    }
    __syncthreads();
    // ---- order: (distance, position); a non-finite distance makes the entry empty (after the dedupe: it still shadowed its repeats)
    for (int p = tid; p < P; p += LINK_NT) s_key[p] = (p < K && s_id[p] >= 0 && insert_finite(s_d[p])) ? make_key(s_d[p], p) : KEY_NONE;
    __syncthreads();
    sort_keys<LINK_NT>(s_key, P, tid);
    for (int j = tid; j < K; j += LINK_NT) {
        const uint64_t key = s_key[j];
        const int p = key == KEY_NONE ? 0 : key_id(key);
        oc[j] = key == KEY_NONE ? -1 : s_id[p];
        od[j] = key == KEY_NONE ? __builtin_inff() : s_d[p];
    }
}

// One wave per batch row: edges i m + r (v -> u) and b m + i m + r (u -> v) for the r-th kept candidate, the invalid pair for every other
// r < m; then, in refinement, row v := empty.  The candidates were formed by an earlier launch, so the clearing cannot reach their reads.
__global__ __launch_bounds__(LINK_NT) void k_insert_edges(const int32_t* batch, int64_t b, int64_t n, int K, int m, const int32_t* cand, const float* cdist,
                                                          const uint8_t* keep, int32_t* src, int32_t* dst, float* w, int replace, int cap, int32_t* adj, float* dist,
                                                          int32_t* deg) {
    const int lane = threadIdx.x;
    const int64_t i = blockIdx.x;
    const int32_t v = batch[i];
    const bool live = v >= 0 && (int64_t)v < n;
    const int64_t f0 = i * m, r0 = b * m + i * m;
    int base = 0;
    for (int c0 = 0; c0 < K; c0 += 64) {
        const int c = c0 + lane;
        const bool kept = live && c < K && keep[i * K + c] != 0;
        const unsigned long long mask = __ballot(kept);
        const int r = base + __popcll(mask & ((1ull << lane) - 1ull));
        if (kept && r < m) {
            const int32_t u = cand[i * K + c];
            const float x = cdist[i * K + c];
            src[f0 + r] = v;
            dst[f0 + r] = u;
            w[f0 + r] = x;
            src[r0 + r] = u;
            dst[r0 + r] = v;
            w[r0 + r] = x;
        }
        base += __popcll(mask);
    }
    for (int r = min(base, m) + lane; r < m; r += 64) {
        src[f0 + r] = -1;
        dst[f0 + r] = -1;
        w[f0 + r] = 0.0f;
        src[r0 + r] = -1;
        dst[r0 + r] = -1;
        w[r0 + r] = 0.0f;
    }
    if (replace && live) {
        for (int c = lane; c < cap; c += 64) {
            adj[(int64_t)v * cap + c] = -1;
            dist[(int64_t)v * cap + c] = __builtin_inff();
        }
        if (lane == 0) deg[v] = 0;
    }
}

}  // namespace lm

extern "C" {

int lm_graph_insert_batch(lm_index* ix, const int32_t* d_batch, int64_t b, int32_t replace, int32_t kk, int32_t m, float alpha, const lm_search_params* params,
                          int32_t* d_adj, float* d_dist, int32_t* d_deg, int32_t* d_cand_out, float* d_cdist_out, uint8_t* d_keep_out) {
    using namespace lm;
    // ---- everything that is refused, in front of any allocation, staging or launch
    if (!ix || !params) LM_FAIL(LM_EINVAL, "NULL index or params");
    if (!ix->view) LM_FAIL(LM_ESTATE, "lm_graph_insert_batch needs a view index (lm_index_create_view)");
    if (!ix->d_table) LM_FAIL(LM_ESTATE, "lm_graph_insert_batch needs a stored-embedding table (lm_index_attach_table)");
    if (b < 0) LM_FAIL(LM_EINVAL, "b must not be negative");
    if (b > 0 && !d_batch) LM_FAIL(LM_EINVAL, "d_batch is NULL");
    if (replace != 0 && replace != 1) LM_FAIL(LM_EINVAL, "replace must be 0 or 1");
    if (kk < 1 || m < 1) LM_FAIL(LM_EINVAL, "kk and m must be >= 1");
    const int32_t cap = ix->view_levels[0].cap;
    const int64_t K = (int64_t)kk + (replace ? cap : 0);
    if (K > LM_SELECT_MAX_K) LM_FAIL(LM_EINVAL, "K = kk (+ levels[0].cap when replace) must be <= LM_SELECT_MAX_K = " + std::to_string(LM_SELECT_MAX_K));
    if (b > 0x7fffffffll / 2 / m) LM_FAIL(LM_EINVAL, "2 * b * m edges exceed INT32_MAX");
    if (int rc = link_check_params(ix->table_dtype, ix->Dp, ix->metric, cap, alpha)) return rc;
    if (!d_dist || !d_deg || (ix->N > 0 && !d_adj)) LM_FAIL(LM_EINVAL, "NULL level array");
    if (d_adj != ix->view_levels[0].d_adj) LM_FAIL(LM_EINVAL, "d_adj is not the view's level-0 array: the search would not see what the links change");
    if (params->efSearch <= 0) LM_FAIL(LM_EINVAL, "efSearch must be positive");
    if (params->batch_size < 0) LM_FAIL(LM_EINVAL, "batch_size must not be negative (0 = no dynamic batching)");
    if (int vrc = view_checks(ix, 1, kk, params)) return vrc;  // (with one query: its refusals do not depend on the number)
    if (b == 0) return LM_OK;

    LM_HIP(hipSetDevice(ix->device));
    const int64_t ne = 2 * b * m;
    const size_t bK = (size_t)b * (size_t)K;
    int rc;
    if ((rc = ix->d_ins_q.reserve((size_t)b * ix->D)) || (rc = ix->d_ins_sd.reserve((size_t)b * kk)) || (rc = ix->d_ins_sl.reserve((size_t)b * kk)) ||
        (rc = ix->d_ins_cand.reserve(bK)) || (rc = ix->d_ins_cdist.reserve(bK)) || (rc = ix->d_ins_keep.reserve(bK)) || (rc = ix->d_ins_src.reserve((size_t)ne)) ||
        (rc = ix->d_ins_dst.reserve((size_t)ne)) || (rc = ix->d_ins_w.reserve((size_t)ne)) ||
        (rc = ix->d_ins_ws.reserve(lm_graph_add_links_workspace_bytes(ix->N, ne))))
        return rc;
    hipStream_t st = ix->stream;
    float* q = ix->d_ins_q.get();
    float* sd = ix->d_ins_sd.get();
    int64_t* sl = ix->d_ins_sl.get();
    int32_t* cand = ix->d_ins_cand.get();
    float* cdist = ix->d_ins_cdist.get();
    uint8_t* keep = ix->d_ins_keep.get();
    const bool f16 = ix->table_dtype == LM_DTYPE_F16;
    hipLaunchKernelGGL(k_insert_queries, dim3((unsigned)((b * ix->D + 255) / 256)), dim3(256), 0, st, (const void*)ix->d_table, f16 ? 1 : 0, ix->N, (int)ix->D, (int)ix->Dp,
                       d_batch, b, q);
    LM_HIP(hipGetLastError());
    if ((rc = do_search_device(ix, b, q, kk, sd, sl, params)) != LM_OK) return rc;
    hipLaunchKernelGGL(k_insert_merge, dim3((unsigned)b), dim3(LINK_NT), 0, st, (const int64_t*)sl, (const float*)sd, ix->metric == LM_METRIC_L2 ? 1 : 0, d_batch, ix->N,
                       (int)kk, (int)replace, (int)cap, (const int32_t*)d_adj, (const float*)d_dist, cand, cdist);
    LM_HIP(hipGetLastError());
    if (ix->N == 0) {  // every row is void: no candidate, nothing to select or link
        LM_HIP(hipMemsetAsync(keep, 0, bK, st));
    } else if ((rc = select_launch(ix->d_table, ix->table_dtype, ix->N, ix->Dp, ix->metric, cand, cdist, b, (int32_t)K, m, alpha, keep, st)) != LM_OK) {
        return rc;
    }
    if (d_cand_out) LM_HIP(hipMemcpyAsync(d_cand_out, cand, bK * 4, hipMemcpyDeviceToDevice, st));
    if (d_cdist_out) LM_HIP(hipMemcpyAsync(d_cdist_out, cdist, bK * 4, hipMemcpyDeviceToDevice, st));
    if (d_keep_out) LM_HIP(hipMemcpyAsync(d_keep_out, keep, bK, hipMemcpyDeviceToDevice, st));
    if (ix->N == 0) return LM_OK;
    hipLaunchKernelGGL(k_insert_edges, dim3((unsigned)b), dim3(LINK_NT), 0, st, d_batch, b, ix->N, (int)K, (int)m, (const int32_t*)cand, (const float*)cdist,
                       (const uint8_t*)keep, ix->d_ins_src.get(), ix->d_ins_dst.get(), ix->d_ins_w.get(), (int)replace, (int)cap, d_adj, d_dist, d_deg);
    LM_HIP(hipGetLastError());
    return link_launch(ix->d_table, ix->table_dtype, ix->Dp, ix->metric, d_adj, d_dist, d_deg, ix->N, cap, ix->d_ins_src.get(), ix->d_ins_dst.get(), ix->d_ins_w.get(), ne,
                       alpha, ix->d_ins_ws.get(), st);
}

}  // extern "C"
