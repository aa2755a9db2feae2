// lm_link_impl.h -- index build time: the link insertion of graph construction (faiss HNSW::add_link / shrink_neighbor_list run over a
// whole batch of directed edges at once): merge the new edges into the affected rows of a fixed-capacity adjacency, dedupe by target,
// order by (distance, id), shrink overflowing rows with the select-neighbours rule.  Included at the end of lm_search.hip after
// lm_select_impl.h (shares load_row / row_reduce / make_key / SELECT_WORDS: the shrink is k_select_neighbors' scan on the same canonical
// distances); include/leann_mi355x.h states the contract, tests/link_ref/lm_link_ref.c restates it.
//
// Reference surface replaced: index.add of leann_backend_hnsw/hnsw_backend.py:66-94 (faiss links every inserted node and its reverse
// edges this way), leann_amd/gpu_graph_build.py's torch form of it (_LevelGraph.add_links: unique, three sorts, bincount, cumsum,
// scatters and a host synchronisation per call).
//
// Shape: four launches.
//   k_link_count   one lane per edge: integer atomicAdd on the source row's counter (a count does not depend on arrival order);
//   k_link_scan    one workgroup: exclusive scan of the counters, tile by tile (wave shuffles + one LDS hand-over per tile); it also
//                  clears the counters, which the next kernel uses as cursors, and lists the affected rows in ascending order (the same
//                  scan over the flags count > 0), so that the row kernel's grid is min(n, ne) workgroups, not n;
//   k_link_fill    one lane per edge: (edge index, dst, w) into the source row's bucket.  The ORDER inside a bucket depends on how the
//                  atomics land; nothing later does: every decision below is taken on the total key (distance, dst, edge index);
//   k_link_row     one workgroup per affected row (workgroup b takes the b-th affected row; those beyond the list leave at once).  A candidate is a WINNER when no candidate of the same dst precedes it (existing
//                  slots in slot order, then edges by index).  Winners have distinct dsts, hence distinct (distance, dst) keys, and the
//                  row's new list is the select rule over the 2 cap smallest of them.  The pool of winners lives in LDS: the existing
//                  row's, then the bucket in pieces of LM_LINK_STAGE edges; after every piece the pool is cut back to its 2 cap best by
//                  counting ranks (keys are distinct: a rank is a place, no sort), and from then on an edge is looked at only if its key
//                  is below the pool's last -- so a hub with thousands of reverse links pays the all-pairs duplicate test for the few
//                  edges that can still enter.  A bucket of any size is exact: the duplicate test always scans the whole bucket.
#pragma once

namespace lm {

constexpr int LINK_NT = 64;                        // lanes per row workgroup: one wave (its barriers cost next to nothing, and the shrink
                                                   // scan, which runs on one 16-lane group as in k_select_neighbors, idles 48 lanes, not 240)
constexpr int LINK_MAX_CAP = LM_SELECT_MAX_K / 2;  // cap: 2 cap candidates go through the K-bit mask of the select scan
constexpr int LINK_POOL = LM_SELECT_MAX_K + LM_LINK_STAGE;
constexpr int LINK_SCAN_NT = 1024;

__device__ __forceinline__ bool link_edge_ok(int32_t s, int32_t d, int64_t n) { return s >= 0 && (int64_t)s < n && d >= 0 && (int64_t)d < n && s != d; }

__global__ __launch_bounds__(256) void k_link_count(const int32_t* src, const int32_t* dst, int64_t ne, int64_t n, int32_t* cnt) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= ne) return;
    const int32_t s = src[e], d = dst[e];
    if (link_edge_ok(s, d, n)) atomicAdd(&cnt[s], 1);
}

// start[v] = number of valid edges of the rows below v; rows[0 .. rows[n]) = the rows with a valid edge, ascending; cnt[v] = 0
// afterwards.  One workgroup walks the rows in tiles of LINK_SCAN_NT.
__global__ __launch_bounds__(LINK_SCAN_NT) void k_link_scan(int32_t* cnt, int32_t* start, int32_t* rows, int64_t n) {
    __shared__ int32_t s_wave[LINK_SCAN_NT / 64], s_wavef[LINK_SCAN_NT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int32_t carry = 0, carryf = 0;
    for (int64_t base = 0; base < n; base += LINK_SCAN_NT) {
        const int64_t v = base + tid;
        const int32_t c = v < n ? cnt[v] : 0;
        const int32_t f = c > 0 ? 1 : 0;
        int32_t incl = c, inclf = f;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int32_t up = __shfl_up(incl, d), upf = __shfl_up(inclf, d);
            if (lane >= d) {
                incl += up;
                inclf += upf;
            }
        }
        if (lane == 63) {
            s_wave[wave] = incl;
            s_wavef[wave] = inclf;
        }
        __syncthreads();
        int32_t below = 0, total = 0, belowf = 0, totalf = 0;
#pragma unroll
        for (int w = 0; w < LINK_SCAN_NT / 64; ++w) {
            const int32_t t = s_wave[w], tf = s_wavef[w];
            below += w < wave ? t : 0;
            total += t;
            belowf += w < wave ? tf : 0;
            totalf += tf;
        }
        if (v < n) {
            start[v] = carry + below + incl - c;
            cnt[v] = 0;  // the fill counts up again: its cursor, and afterwards the bucket's size
            if (f) rows[carryf + belowf + inclf - 1] = (int32_t)v;
        }
        carry += total;
        carryf += totalf;
        __syncthreads();  // s_wave / s_wavef are rewritten by the next tile
    }
    if (tid == 0) rows[n] = carryf;  // how many rows are affected
}

__global__ __launch_bounds__(256) void k_link_fill(const int32_t* src, const int32_t* dst, const float* w, int64_t ne, int64_t n, int32_t* cur,
                                                   const int32_t* start, int32_t* b_dst, int32_t* b_e, float* b_w) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= ne) return;
    const int32_t s = src[e], d = dst[e];
    if (!link_edge_ok(s, d, n)) return;
    const int64_t p = (int64_t)start[s] + atomicAdd(&cur[s], 1);
    b_dst[p] = d;
    b_e[p] = (int32_t)e;
    b_w[p] = w[e];
}

template <int NCH, bool L2, bool F16>
__global__ __launch_bounds__(LINK_NT) void k_link_row(const void* table, int32_t* adj, float* dist, int32_t* deg, int64_t n, int cap, const int32_t* cnt,
                                                       const int32_t* start, const int32_t* rows, const int32_t* b_dst, const int32_t* b_e, const float* b_w, float a2,
                                                       int relaxed) {
    __shared__ uint64_t s_key[2][LINK_POOL];  // the pool of winners, (distance, dst) keys; buffer `cur` is the live one
    __shared__ float s_w[2][LINK_POOL];       // their weights as given (the key canonicalises NaN and -0: the stored distance must not)
    __shared__ int32_t s_ex[LINK_MAX_CAP];    // the existing row's ids (-1: empty slot)
    __shared__ int32_t s_sd[LM_LINK_STAGE];   // a bucket that fits: its dsts and edge indices, for the duplicate test
    __shared__ int32_t s_se[LM_LINK_STAGE];
    __shared__ int s_n;                       // entries in the live buffer
    __shared__ int s_no;                      // entries of s_out
    __shared__ int32_t s_out[LINK_MAX_CAP];   // the shrunk row: positions in the pool, in order
    const int tid = threadIdx.x;
    if ((int64_t)blockIdx.x >= (int64_t)rows[n]) return;  // beyond the list of affected rows (the whole workgroup leaves)
    const int64_t v = rows[blockIdx.x];  // rows that are not listed are not written at all
    const int m = cnt[v];
    const int K2 = 2 * cap;
    const int64_t b0 = start[v];
    int32_t* arow = adj + v * cap;
    float* drow = dist + v * cap;

    // ---- existing entries: the first slot of every id enters the pool
    if (tid == 0) s_n = 0;
    for (int c = tid; c < cap; c += LINK_NT) {
        const int32_t id = arow[c];
        s_ex[c] = (id >= 0 && (int64_t)id < n) ? id : -1;
    }
    const bool staged = m <= LM_LINK_STAGE;
    if (staged)
        for (int i = tid; i < m; i += LINK_NT) {
            s_sd[i] = b_dst[b0 + i];
            s_se[i] = b_e[b0 + i];
        }
    __syncthreads();
    for (int c = tid; c < cap; c += LINK_NT) {
        const int32_t id = s_ex[c];
        if (id < 0) continue;
        bool first = true;
        for (int x = 0; x < c; ++x) first &= s_ex[x] != id;
        if (!first) continue;
        const float w = drow[c];
        const int p = atomicAdd(&s_n, 1);
        s_key[0][p] = make_key(w, id);
        s_w[0][p] = w;
    }
    __syncthreads();

    // ---- the bucket, LM_LINK_STAGE edges at a time
    int cur = 0;
    uint64_t thr = KEY_NONE;  // once the pool is full: its largest key; an edge at or above it cannot be among the 2 cap best winners
    for (int c0 = 0; c0 < m; c0 += LM_LINK_STAGE) {
        const int c1 = min(m, c0 + LM_LINK_STAGE);
        for (int i = c0 + tid; i < c1; i += LINK_NT) {
            const int32_t d = staged ? s_sd[i] : b_dst[b0 + i];
            const float w = b_w[b0 + i];
            const uint64_t key = make_key(w, d);
            if (key >= thr) continue;
            bool win = true;
            for (int x = 0; x < cap; ++x) win &= s_ex[x] != d;  // an existing entry beats any incoming edge
            if (!win) continue;
            const int32_t e = staged ? s_se[i] : b_e[b0 + i];
            if (staged) {
                for (int x = 0; x < m; ++x) win &= !(s_sd[x] == d && s_se[x] < e);
            } else {
                // among incoming edges the lowest index wins.  No early exit: independent loads that the compiler can keep in flight
                for (int x = 0; x < m; ++x) win &= !((b_dst[b0 + x] == d) & (b_e[b0 + x] < e));
            }
            if (!win) continue;
            const int p = atomicAdd(&s_n, 1);  // at most 2 cap + LM_LINK_STAGE entries: the pool was cut to 2 cap before this piece
            s_key[cur][p] = key;
            s_w[cur][p] = w;
        }
        __syncthreads();
        const int pn = s_n;
        __syncthreads();  // every lane has read the count before the next piece (or lane 0 below) moves it
        const bool last = c1 == m;
        if (pn > K2 || last) {  // rank = place: keys are distinct
            for (int i = tid; i < pn; i += LINK_NT) {
                const uint64_t key = s_key[cur][i];
                int below = 0;
                for (int x = 0; x < pn; ++x) below += s_key[cur][x] < key ? 1 : 0;
                if (below < K2) {
                    s_key[cur ^ 1][below] = key;
                    s_w[cur ^ 1][below] = s_w[cur][i];
                }
            }
            __syncthreads();
            cur ^= 1;
            if (tid == 0) s_n = min(pn, K2);
            if (pn >= K2) thr = s_key[cur][K2 - 1];
            __syncthreads();
        }
    }
    const int pc = s_n;  // the candidates: s_key[cur][0 .. pc), ascending
    const uint64_t* ck = s_key[cur];
    const float* cw = s_w[cur];

    // ---- at most cap: the list as it stands
    if (pc <= cap) {
        for (int c = tid; c < cap; c += LINK_NT) {
            arow[c] = c < pc ? key_id(ck[c]) : -1;
            drow[c] = c < pc ? cw[c] : __builtin_inff();
        }
        if (tid == 0) deg[v] = pc;
        return;
    }

    // ---- more: k_select_neighbors' scan (K = 2 cap, m = cap) by one 16-lane group, candidates and distances from LDS
    if (tid < 16) {
        const int lane16 = tid;
        uint64_t kept[SELECT_WORDS];
#pragma unroll
        for (int w = 0; w < SELECT_WORDS; ++w) kept[w] = 0;
        int nk = 0;
        float4 cv[NCH], e[NCH];
        for (int pass = 0; pass <= relaxed; ++pass) {
            for (int j = 0; j < pc && nk < cap; ++j) {
                bool mine = false;
#pragma unroll
                for (int w = 0; w < SELECT_WORDS; ++w) mine |= (j >> 6) == w && ((kept[w] >> (j & 63)) & 1ull);
                if (mine) continue;
                float t = cw[j];
                if (pass) t = L2 ? t / a2 : -(1.0f - (1.0f + t) / a2);
                load_row<NCH, F16>(table, key_id(ck[j]), lane16, cv);
                bool dominated = false;
#pragma unroll
                for (int w = 0; w < SELECT_WORDS; ++w) {
                    uint64_t bits = kept[w];
                    while (bits && !dominated) {
                        const int i = w * 64 + __builtin_ctzll(bits);
                        bits &= bits - 1;
                        load_row<NCH, F16>(table, key_id(ck[i]), lane16, e);
                        if (row_reduce<NCH, L2>(e, cv) <= t) dominated = true;  // plain IEEE: NaN never dominates
                    }
                }
                if (!dominated) {
#pragma unroll
                    for (int w = 0; w < SELECT_WORDS; ++w)
                        if ((j >> 6) == w) kept[w] |= 1ull << (j & 63);
                    ++nk;
                }
            }
        }
        if (lane16 == 0) {
            int o = 0;
#pragma unroll
            for (int w = 0; w < SELECT_WORDS; ++w) {
                uint64_t bits = kept[w];
                while (bits) {
                    s_out[o++] = w * 64 + __builtin_ctzll(bits);
                    bits &= bits - 1;
                }
            }
            s_no = o;
        }
    }
    __syncthreads();
    const int no = s_no;
    for (int c = tid; c < cap; c += LINK_NT) {
        arow[c] = c < no ? key_id(ck[s_out[c]]) : -1;
        drow[c] = c < no ? cw[s_out[c]] : __builtin_inff();
    }
    if (tid == 0) deg[v] = no;
}

inline size_t link_align(size_t b) { return (b + 255) & ~(size_t)255; }

// what lm_graph_add_links and lm_graph_prune_hubs (lm_prune_impl.h) reject alike: the table's layout, the metric, cap, alpha
inline int link_check_params(int32_t dtype, int32_t d_padded, int32_t metric, int32_t cap, float alpha) {
    if (d_padded <= 0 || d_padded % 64) LM_FAIL(LM_EINVAL, "d_padded must be a positive multiple of 64");
    switch (d_padded / 64) {
        case 1: case 2: case 3: case 4: case 5: case 6: case 8: case 12: case 16: break;
        default: LM_FAIL(LM_EINVAL, "unsupported padded dimension (supported: 64..384, 512, 768, 1024)");
    }
    if (dtype != LM_DTYPE_F32 && dtype != LM_DTYPE_F16) LM_FAIL(LM_EINVAL, "dtype must be f32 or f16");
    if (metric != LM_METRIC_INNER_PRODUCT && metric != LM_METRIC_L2) LM_FAIL(LM_EINVAL, "unknown metric");
    if (cap < 1 || cap > LINK_MAX_CAP) LM_FAIL(LM_EINVAL, "cap must be in [1, LM_SELECT_MAX_K / 2 = " + std::to_string(LINK_MAX_CAP) + "]");
    if (!std::isfinite(alpha) || alpha < 1.0f) LM_FAIL(LM_EINVAL, "alpha must be finite and >= 1");
    return LM_OK;
}

// the launch sequence of lm_graph_add_links on checked arguments (n, ne in [1, INT32_MAX], a workspace of at least
// lm_graph_add_links_workspace_bytes(n, ne)): both entry points enqueue exactly this
inline int link_launch(const void* d_table, int32_t dtype, int32_t d_padded, int32_t metric, int32_t* d_adj, float* d_dist, int32_t* d_deg, int64_t n, int32_t cap,
                       const int32_t* d_src, const int32_t* d_dst, const float* d_w, int64_t ne, float alpha, void* d_workspace, hipStream_t st) {
    char* ws = (char*)d_workspace;
    int32_t* cnt = (int32_t*)ws;
    int32_t* start = (int32_t*)(ws + link_align((size_t)n * 4));
    int32_t* rows = (int32_t*)(ws + 2 * link_align((size_t)n * 4));
    char* bk = ws + 2 * link_align((size_t)n * 4) + link_align(((size_t)n + 1) * 4);
    int32_t* b_dst = (int32_t*)bk;
    int32_t* b_e = (int32_t*)(bk + link_align((size_t)ne * 4));
    float* b_w = (float*)(bk + 2 * link_align((size_t)ne * 4));
    LM_HIP(hipMemsetAsync(cnt, 0, (size_t)n * 4, st));
    const dim3 egrid((unsigned)((ne + 255) / 256));
    hipLaunchKernelGGL(k_link_count, egrid, dim3(256), 0, st, d_src, d_dst, ne, n, cnt);
    hipLaunchKernelGGL(k_link_scan, dim3(1), dim3(LINK_SCAN_NT), 0, st, cnt, start, rows, n);
    hipLaunchKernelGGL(k_link_fill, egrid, dim3(256), 0, st, d_src, d_dst, d_w, ne, n, cnt, (const int32_t*)start, b_dst, b_e, b_w);
    const float a2 = alpha * alpha;
    const int relaxed = alpha != 1.0f ? 1 : 0;
    const dim3 rgrid((unsigned)std::min(n, ne)), rblock(LINK_NT);  // an affected row has a valid edge: at most min(n, ne) of them (<= INT32_MAX, HIP's grid limit)
    const bool l2 = metric == LM_METRIC_L2, f16 = dtype == LM_DTYPE_F16;
#define LM_LINK_ARGS d_table, d_adj, d_dist, d_deg, n, (int)cap, (const int32_t*)cnt, (const int32_t*)start, (const int32_t*)rows, (const int32_t*)b_dst, (const int32_t*)b_e, (const float*)b_w, a2, relaxed
#define GO(nch)                                                                                                     \
    case nch:                                                                                                       \
        if (l2 && f16) hipLaunchKernelGGL((k_link_row<nch, true, true>), rgrid, rblock, 0, st, LM_LINK_ARGS);       \
        else if (l2) hipLaunchKernelGGL((k_link_row<nch, true, false>), rgrid, rblock, 0, st, LM_LINK_ARGS);        \
        else if (f16) hipLaunchKernelGGL((k_link_row<nch, false, true>), rgrid, rblock, 0, st, LM_LINK_ARGS);       \
        else hipLaunchKernelGGL((k_link_row<nch, false, false>), rgrid, rblock, 0, st, LM_LINK_ARGS);               \
        break
    switch (d_padded / 64) {
        GO(1); GO(2); GO(3); GO(4); GO(5); GO(6); GO(8); GO(12); GO(16);
    }
#undef GO
#undef LM_LINK_ARGS
    LM_HIP(hipGetLastError());
    return LM_OK;
}

}  // namespace lm

extern "C" {

// workspace: counters / cursors [n], bucket starts [n], affected rows [n] + their number, then the buckets: dst, edge index, weight [ne] each
size_t lm_graph_add_links_workspace_bytes(int64_t n, int64_t ne) {
    if (n < 0 || ne < 0 || n > 0x7fffffffll || ne > 0x7fffffffll) return 0;
    if (n == 0 || ne == 0) return 0;
    return 2 * lm::link_align((size_t)n * 4) + lm::link_align(((size_t)n + 1) * 4) + 3 * lm::link_align((size_t)ne * 4);
}

int lm_graph_add_links(const void* d_table, int32_t dtype, int32_t d_padded, int32_t metric, int32_t* d_adj, float* d_dist, int32_t* d_deg, int64_t n,
                       int32_t cap, const int32_t* d_src, const int32_t* d_dst, const float* d_w, int64_t ne, float alpha, void* d_workspace,
                       size_t workspace_bytes, void* stream) {
    using namespace lm;
    if (int rc = link_check_params(dtype, d_padded, metric, cap, alpha)) return rc;
    if (n < 0 || ne < 0 || n > 0x7fffffffll || ne > 0x7fffffffll) LM_FAIL(LM_EINVAL, "n / ne must be in [0, INT32_MAX]");
    if (n == 0 || ne == 0) return LM_OK;
    if (!d_table || !d_adj || !d_dist || !d_deg || !d_src || !d_dst || !d_w || !d_workspace) LM_FAIL(LM_EINVAL, "NULL buffer");
    if ((uintptr_t)d_workspace % 4) LM_FAIL(LM_EINVAL, "d_workspace must be 4-byte aligned");
    if (workspace_bytes < lm_graph_add_links_workspace_bytes(n, ne)) LM_FAIL(LM_EINVAL, "workspace smaller than lm_graph_add_links_workspace_bytes(n, ne)");
    return link_launch(d_table, dtype, d_padded, metric, d_adj, d_dist, d_deg, n, cap, d_src, d_dst, d_w, ne, alpha, d_workspace, (hipStream_t)stream);
}

}  // extern "C"
