// lm_prune_impl.h -- index build time: high-degree-preserving pruning of the level-0 graph (LEANN paper, Algorithm 3) as one library
// call: count in-degrees, pick the hubs under the total order (in-degree descending, id ascending), keep the first quota[v] usable links
// of every row, offer every kept link in both directions with its canonical distance, and hand these edges -- ONCE -- to the link
// insertion on an empty graph.  Included at the end of lm_search.hip after lm_link_impl.h (link_launch is lm_graph_add_links' launch
// sequence, unchanged; load_row / row_reduce give the canonical distance); include/leann_mi355x.h states the contract,
// tests/prune_ref/lm_prune_ref.c restates it.
//
// Reference surface replaced: leann_amd/gpu_graph_build.py's host form of the pruning (prune_preserving_hubs: an int64 [n, 2M] numpy
// array, np.bincount, np.argpartition -- ties at the cut broken arbitrarily --, a torch sum for the weights, add_links in chunks).
//
// Shape: everything is enqueued on the caller's stream, nothing comes back to the host.
//   k_prune_fill      the outputs := empty (-1, +inf, 0);
//   k_prune_indeg     one lane per slot: integer atomicAdd on the target's counter;
//   k_prune_hist /    radix select of the n_hubs-th largest in-degree T, most significant byte first: a 256-bin histogram per workgroup
//   k_prune_pick      in LDS, one global add per non-empty bin (same-address atomics serialise in the L2), then one lane walks the bins
//                     from the top and fixes the next byte of T; after four bytes: T, and how many nodes AT T are hubs (those of
//                     lowest id);
//   k_prune_scan      one workgroup, tile by tile as k_link_scan: the rank of every node among those at T in id order decides who is a
//                     hub; base[] = exclusive scan of the quotas; the hubs' (in-degree, id) keys are listed in id order;
//   k_prune_sort_*    only when the caller wants the hub list: bitonic sort of those keys (steps below SORT_TILE in LDS);
//   k_prune_emit      one 16-lane group per kept link (v, r): edges 2j and 2j + 1, j = base[v] + r, or the invalid pair when row v has
//                     fewer than r + 1 usable slots.  Two launches: r < min(m_low, cap) for all rows, the remaining r for the hubs;
//   link_launch       lm_graph_add_links' four kernels on these edges.
#pragma once

namespace lm {

constexpr int PRUNE_SORT_TILE = 512;  // keys per workgroup of the LDS sort steps (256 lanes, two keys each)
constexpr int PRUNE_HIST_MAX_BLOCKS = 2048;

__device__ __forceinline__ bool prune_usable(int32_t u, int64_t v, int64_t n) { return u >= 0 && (int64_t)u < n && (int64_t)u != v; }
// hubs sort ascending on this: in-degree descending (0 <= indeg <= INT32_MAX), then id ascending
__device__ __forceinline__ uint64_t prune_hub_key(int32_t indeg, int64_t v) { return ((uint64_t)(uint32_t)(0x7fffffff - indeg) << 32) | (uint64_t)(uint32_t)v; }

__global__ __launch_bounds__(256) void k_prune_fill(int32_t* adj, float* dist, int32_t* deg, int64_t n, int cap) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < n * cap) {
        adj[t] = -1;
        dist[t] = __builtin_inff();
    }
    if (t < n) deg[t] = 0;
}

__global__ __launch_bounds__(256) void k_prune_indeg(const int32_t* adj, int64_t n, int cap, int32_t* indeg) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n * cap) return;
    const int32_t u = adj[t];
    if (prune_usable(u, t / cap, n)) atomicAdd(&indeg[u], 1);
}

// state[0]: the bytes of T fixed so far (those above `shift` + 8), state[1]: how many hubs are still to be found among the nodes that
// match them.  hist[0 .. 256): byte (x >> shift) & 255 of every in-degree x that matches.
__global__ __launch_bounds__(256) void k_prune_hist(const int32_t* indeg, int64_t n, const int32_t* state, int shift, int32_t* hist) {
    __shared__ int32_t s_h[256];
    const int tid = threadIdx.x;
    s_h[tid] = 0;
    __syncthreads();
    const uint32_t prefix = shift == 24 ? 0u : (uint32_t)state[0] >> (shift + 8);
    for (int64_t v = (int64_t)blockIdx.x * 256 + tid; v < n; v += (int64_t)gridDim.x * 256) {
        const uint32_t x = (uint32_t)indeg[v];
        if (shift == 24 || (x >> (shift + 8)) == prefix) atomicAdd(&s_h[(x >> shift) & 255u], 1);
    }
    __syncthreads();
    const int32_t c = s_h[tid];
    if (c) atomicAdd(&hist[tid], c);
}

// n_hubs == 0: T = INT32_MAX with no node taken at T (an in-degree is never above it)
__global__ __launch_bounds__(64) void k_prune_pick(const int32_t* hist, int32_t* state, int shift, int32_t n_hubs) {
    if (threadIdx.x != 0) return;
    if (n_hubs == 0) {
        state[0] = 0x7fffffff;
        state[1] = 0;
        return;
    }
    int32_t k = shift == 24 ? n_hubs : state[1];
    const uint32_t prefix = shift == 24 ? 0u : (uint32_t)state[0];
    int b = 255;
    for (; b > 0; --b) {  // the matching nodes number at least k: the walk ends at bin 0 at the latest
        const int32_t h = hist[b];
        if (h >= k) break;
        k -= h;
    }
    state[0] = (int32_t)(prefix | ((uint32_t)b << shift));
    state[1] = k;
}

// exclusive prefix of (a, b) over the workgroup's lanes plus the carries; the carries move on by the tile's totals.  Two barriers.
__device__ __forceinline__ void prune_scan2(int32_t a, int32_t b, int32_t& carry_a, int32_t& carry_b, int32_t* s_a, int32_t* s_b, int32_t& ex_a, int32_t& ex_b) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int32_t ia = a, ib = b;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int32_t ua = __shfl_up(ia, d), ub = __shfl_up(ib, d);
        if (lane >= d) {
            ia += ua;
            ib += ub;
        }
    }
    if (lane == 63) {
        s_a[wave] = ia;
        s_b[wave] = ib;
    }
    __syncthreads();
    int32_t below_a = 0, total_a = 0, below_b = 0, total_b = 0;
#pragma unroll
    for (int w = 0; w < LINK_SCAN_NT / 64; ++w) {
        const int32_t ta = s_a[w], tb = s_b[w];
        below_a += w < wave ? ta : 0;
        total_a += ta;
        below_b += w < wave ? tb : 0;
        total_b += tb;
    }
    ex_a = carry_a + below_a + ia - a;
    ex_b = carry_b + below_b + ib - b;
    carry_a += total_a;
    carry_b += total_b;
    __syncthreads();  // s_a / s_b are rewritten by the next scan
}

// base[v] = sum of the quotas below v (base[n]: all of them); keys[0 .. n_hubs) = the hubs' keys in id order, keys[n_hubs .. P) = none;
// indeg_out (optional) = the in-degrees.
__global__ __launch_bounds__(LINK_SCAN_NT) void k_prune_scan(const int32_t* indeg, int64_t n, const int32_t* state, int cap, int mq, int32_t* base, uint64_t* keys,
                                                             int64_t n_hubs, int64_t P, int32_t* indeg_out) {
    __shared__ int32_t s_a[LINK_SCAN_NT / 64], s_b[LINK_SCAN_NT / 64];
    const int tid = threadIdx.x;
    const int32_t T = state[0], kr = state[1];
    int32_t carry_eq = 0, carry_z = 0, carry_q = 0, carry_h = 0;
    for (int64_t t0 = 0; t0 < n; t0 += LINK_SCAN_NT) {
        const int64_t v = t0 + tid;
        const bool in = v < n;
        const int32_t x = in ? indeg[v] : 0;
        const int32_t eq = in && x == T ? 1 : 0;
        int32_t rank_eq, unused;
        prune_scan2(eq, 0, carry_eq, carry_z, s_a, s_b, rank_eq, unused);
        const int32_t hub = in && (x > T || (eq && rank_eq < kr)) ? 1 : 0;
        const int32_t q = in ? (hub ? cap : mq) : 0;
        int32_t ex_q, ex_h;
        prune_scan2(q, hub, carry_q, carry_h, s_a, s_b, ex_q, ex_h);
        if (in) {
            base[v] = ex_q;
            if (hub) keys[ex_h] = prune_hub_key(x, v);
            if (indeg_out) indeg_out[v] = x;
        }
    }
    if (tid == 0) base[n] = carry_q;
    for (int64_t i = n_hubs + tid; i < P; i += LINK_SCAN_NT) keys[i] = KEY_NONE;
}

// bitonic network over keys[0 .. P), P a power of two >= PRUNE_SORT_TILE: the steps (k2, j) with j < PRUNE_SORT_TILE stay inside an
// aligned tile and run in LDS, for k2 = k2lo .. k2hi; the wider steps take one launch each.
__global__ __launch_bounds__(256) void k_prune_sort_local(uint64_t* keys, unsigned k2lo, unsigned k2hi) {
    __shared__ uint64_t s_k[PRUNE_SORT_TILE];
    const unsigned tid = threadIdx.x;
    const uint64_t g0 = (uint64_t)blockIdx.x * PRUNE_SORT_TILE;
    s_k[tid] = keys[g0 + tid];
    s_k[tid + 256] = keys[g0 + tid + 256];
    __syncthreads();
    for (uint64_t k2 = k2lo; k2 <= k2hi; k2 <<= 1) {
        for (unsigned j = k2 > PRUNE_SORT_TILE ? PRUNE_SORT_TILE / 2 : (unsigned)(k2 >> 1); j > 0; j >>= 1) {
            const unsigned i = 2 * tid - (tid & (j - 1));  // the lower partner of the tid-th pair at distance j
            const uint64_t x = s_k[i], y = s_k[i + j];
            const bool up = ((g0 + i) & k2) == 0;
            if ((x > y) == up) {
                s_k[i] = y;
                s_k[i + j] = x;
            }
            __syncthreads();
        }
    }
    keys[g0 + tid] = s_k[tid];
    keys[g0 + tid + 256] = s_k[tid + 256];
}

__global__ __launch_bounds__(256) void k_prune_sort_step(uint64_t* keys, int64_t P, uint64_t k2, uint64_t j) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (uint64_t)P / 2) return;
    const uint64_t i = 2 * t - (t & (j - 1));
    const uint64_t x = keys[i], y = keys[i + j];
    const bool up = (i & k2) == 0;
    if ((x > y) == up) {
        keys[i] = y;
        keys[i + j] = x;
    }
}

__global__ __launch_bounds__(256) void k_prune_hubs_out(const uint64_t* keys, int64_t n_hubs, int32_t* hubs) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < n_hubs) hubs[t] = (int32_t)(uint32_t)keys[t];
}

// group g = (i, r0 + g % rcount): row v = i, or the i-th listed hub; its r-th kept link.  r < quota[v] by construction of the two launches.
template <int NCH, bool L2, bool F16>
__global__ __launch_bounds__(256) void k_prune_emit(const void* table, const int32_t* adj, int64_t n, int cap, const int32_t* base, const uint64_t* list,
                                                    int64_t nlist, int r0, int rcount, int32_t* src, int32_t* dst, float* w) {
    const int lane16 = threadIdx.x & 15;
    const int64_t g = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    if (g >= nlist * rcount) return;  // a whole 16-lane group leaves together
    const int64_t i = g / rcount;
    const int r = r0 + (int)(g % rcount);
    const int64_t v = list ? (int64_t)(uint32_t)list[i] : i;
    const int64_t j = (int64_t)base[v] + r;
    if (j >= (int64_t)base[v + 1]) return;
    const int32_t* arow = adj + v * cap;
    int32_t u = -1;
    for (int c = 0, seen = 0; c < cap; ++c) {  // the r-th usable slot (rows are left-packed as a rule: r + 1 steps)
        const int32_t a = arow[c];
        if (!prune_usable(a, v, n)) continue;
        if (seen++ == r) {
            u = a;
            break;
        }
    }
    if (u < 0) {  // fewer usable slots than the quota: the invalid pair, nothing dereferenced
        if (lane16 < 2) {
            src[2 * j + lane16] = -1;
            dst[2 * j + lane16] = -1;
            w[2 * j + lane16] = 0.0f;
        }
        return;
    }
    float4 qv[NCH], e[NCH];
    load_row<NCH, F16>(table, v, lane16, qv);
    load_row<NCH, F16>(table, u, lane16, e);
    float d = row_reduce<NCH, L2>(e, qv);
    if (d != d) d = __builtin_bit_cast(float, 0x7FC00000u);  // IEEE leaves a computed NaN's sign and payload to the platform: the contract names one
    if (lane16 < 2) {
        src[2 * j + lane16] = lane16 ? u : (int32_t)v;
        dst[2 * j + lane16] = lane16 ? (int32_t)v : u;
        w[2 * j + lane16] = d;
    }
}

inline int64_t prune_pow2(int64_t n_hubs) {
    int64_t p = PRUNE_SORT_TILE;
    while (p < n_hubs) p <<= 1;
    return p;
}
inline int prune_mq(int32_t cap, int32_t m_low) { return m_low < cap ? m_low : cap; }
// ne, or -1 when (n, cap, m_low, n_hubs) is rejected
inline int64_t prune_edges(int64_t n, int32_t cap, int32_t m_low, int64_t n_hubs) {
    if (cap < 1 || cap > LINK_MAX_CAP || m_low < 1 || n < 0 || n > 0x7fffffffll || n_hubs < 0 || n_hubs > n || n * (int64_t)cap > 0x7fffffffll) return -1;
    const int64_t ne = 2 * (n_hubs * cap + (n - n_hubs) * prune_mq(cap, m_low));
    return ne > 0x7fffffffll ? -1 : ne;
}

}  // namespace lm

extern "C" {

// workspace: in-degrees [n], base [n + 1], 4 histograms + the select state, hub keys [P], the edges src / dst / w [ne], then the link
// insertion's own workspace
size_t lm_graph_prune_hubs_workspace_bytes(int64_t n, int32_t cap, int32_t m_low, int64_t n_hubs) {
    using namespace lm;
    const int64_t ne = prune_edges(n, cap, m_low, n_hubs);
    if (ne < 0 || n == 0) return 0;
    return link_align((size_t)n * 4) + link_align(((size_t)n + 1) * 4) + link_align((4 * 256 + 2) * 4) + link_align((size_t)prune_pow2(n_hubs) * 8) +
           3 * link_align((size_t)ne * 4) + lm_graph_add_links_workspace_bytes(n, ne);
}

int lm_graph_prune_hubs(const void* d_table, int32_t dtype, int32_t d_padded, int32_t metric, const int32_t* d_adj_in, int64_t n, int32_t cap, int32_t m_low,
                        int64_t n_hubs, float alpha, int32_t* d_adj_out, float* d_dist_out, int32_t* d_deg_out, int32_t* d_hubs, int32_t* d_indeg,
                        void* d_workspace, size_t workspace_bytes, void* stream) {
    using namespace lm;
    if (int rc = link_check_params(dtype, d_padded, metric, cap, alpha)) return rc;
    if (m_low < 1) LM_FAIL(LM_EINVAL, "m_low must be >= 1");
    if (n < 0 || n > 0x7fffffffll || n * (int64_t)cap > 0x7fffffffll) LM_FAIL(LM_EINVAL, "n must not be negative and n * cap must be <= INT32_MAX");
    if (n_hubs < 0 || n_hubs > n) LM_FAIL(LM_EINVAL, "n_hubs must be in [0, n]");
    const int64_t ne = prune_edges(n, cap, m_low, n_hubs);
    if (ne < 0) LM_FAIL(LM_EINVAL, "2 * (n_hubs * cap + (n - n_hubs) * min(m_low, cap)) edges exceed INT32_MAX");
    if (n == 0) return LM_OK;
    if (!d_table || !d_adj_in || !d_adj_out || !d_dist_out || !d_deg_out || !d_workspace) LM_FAIL(LM_EINVAL, "NULL buffer");
    if (d_adj_out == d_adj_in) LM_FAIL(LM_EINVAL, "d_adj_out must not be d_adj_in");
    if ((uintptr_t)d_workspace % 8) LM_FAIL(LM_EINVAL, "d_workspace must be 8-byte aligned");
    if (workspace_bytes < lm_graph_prune_hubs_workspace_bytes(n, cap, m_low, n_hubs)) LM_FAIL(LM_EINVAL, "workspace smaller than lm_graph_prune_hubs_workspace_bytes(n, cap, m_low, n_hubs)");
    const int mq = prune_mq(cap, m_low);
    const int64_t P = prune_pow2(n_hubs);
    char* ws = (char*)d_workspace;
    int32_t* indeg = (int32_t*)ws;
    ws += link_align((size_t)n * 4);
    int32_t* base = (int32_t*)ws;
    ws += link_align(((size_t)n + 1) * 4);
    int32_t* hist = (int32_t*)ws;
    int32_t* state = hist + 4 * 256;
    ws += link_align((4 * 256 + 2) * 4);
    uint64_t* keys = (uint64_t*)ws;
    ws += link_align((size_t)P * 8);
    int32_t* e_src = (int32_t*)ws;
    ws += link_align((size_t)ne * 4);
    int32_t* e_dst = (int32_t*)ws;
    ws += link_align((size_t)ne * 4);
    float* e_w = (float*)ws;
    ws += link_align((size_t)ne * 4);
    hipStream_t st = (hipStream_t)stream;
    const int64_t slots = n * cap;
    LM_HIP(hipMemsetAsync(indeg, 0, (size_t)n * 4, st));
    LM_HIP(hipMemsetAsync(hist, 0, (4 * 256 + 2) * 4, st));
    const dim3 sgrid((unsigned)((slots + 255) / 256));
    hipLaunchKernelGGL(k_prune_fill, sgrid, dim3(256), 0, st, d_adj_out, d_dist_out, d_deg_out, n, (int)cap);
    hipLaunchKernelGGL(k_prune_indeg, sgrid, dim3(256), 0, st, d_adj_in, n, (int)cap, indeg);
    if (n_hubs == 0) {
        hipLaunchKernelGGL(k_prune_pick, dim3(1), dim3(64), 0, st, (const int32_t*)hist, state, 24, (int32_t)0);
    } else {
        const dim3 hgrid((unsigned)std::min<int64_t>((n + 255) / 256, PRUNE_HIST_MAX_BLOCKS));
        for (int p = 0; p < 4; ++p) {
            const int shift = 24 - 8 * p;
            hipLaunchKernelGGL(k_prune_hist, hgrid, dim3(256), 0, st, (const int32_t*)indeg, n, (const int32_t*)state, shift, hist + 256 * p);
            hipLaunchKernelGGL(k_prune_pick, dim3(1), dim3(64), 0, st, (const int32_t*)(hist + 256 * p), state, shift, (int32_t)n_hubs);
        }
    }
    hipLaunchKernelGGL(k_prune_scan, dim3(1), dim3(LINK_SCAN_NT), 0, st, (const int32_t*)indeg, n, (const int32_t*)state, (int)cap, mq, base, keys, n_hubs, P, d_indeg);
    const bool l2 = metric == LM_METRIC_L2, f16 = dtype == LM_DTYPE_F16;
    // the edges: r < mq of every row, then r in [mq, cap) of the hubs (their keys name them, in whatever order)
    for (int part = 0; part < 2; ++part) {
        const int64_t nlist = part ? n_hubs : n;
        const int r0 = part ? mq : 0, rcount = part ? cap - mq : mq;
        if (nlist == 0 || rcount == 0) continue;
        const uint64_t* list = part ? keys : nullptr;
        const dim3 ggrid((unsigned)((nlist * rcount + 15) / 16));
#define LM_PRUNE_ARGS d_table, d_adj_in, n, (int)cap, (const int32_t*)base, list, nlist, r0, rcount, e_src, e_dst, e_w
#define GO(nch)                                                                                                        \
    case nch:                                                                                                          \
        if (l2 && f16) hipLaunchKernelGGL((k_prune_emit<nch, true, true>), ggrid, dim3(256), 0, st, LM_PRUNE_ARGS);    \
        else if (l2) hipLaunchKernelGGL((k_prune_emit<nch, true, false>), ggrid, dim3(256), 0, st, LM_PRUNE_ARGS);     \
        else if (f16) hipLaunchKernelGGL((k_prune_emit<nch, false, true>), ggrid, dim3(256), 0, st, LM_PRUNE_ARGS);    \
        else hipLaunchKernelGGL((k_prune_emit<nch, false, false>), ggrid, dim3(256), 0, st, LM_PRUNE_ARGS);            \
        break
        switch (d_padded / 64) {
            GO(1); GO(2); GO(3); GO(4); GO(5); GO(6); GO(8); GO(12); GO(16);
        }
#undef GO
#undef LM_PRUNE_ARGS
    }
    if (d_hubs && n_hubs > 0) {  // after the emit launches: they read the keys, the sort moves them (same stream: in order either way)
        hipLaunchKernelGGL(k_prune_sort_local, dim3((unsigned)(P / PRUNE_SORT_TILE)), dim3(256), 0, st, keys, 2u, (unsigned)PRUNE_SORT_TILE);
        for (uint64_t k2 = 2 * PRUNE_SORT_TILE; k2 <= (uint64_t)P; k2 <<= 1) {
            for (uint64_t j = k2 >> 1; j >= PRUNE_SORT_TILE; j >>= 1)
                hipLaunchKernelGGL(k_prune_sort_step, dim3((unsigned)((P / 2 + 255) / 256)), dim3(256), 0, st, keys, P, k2, j);
            hipLaunchKernelGGL(k_prune_sort_local, dim3((unsigned)(P / PRUNE_SORT_TILE)), dim3(256), 0, st, keys, (unsigned)k2, (unsigned)k2);
        }
        hipLaunchKernelGGL(k_prune_hubs_out, dim3((unsigned)((n_hubs + 255) / 256)), dim3(256), 0, st, (const uint64_t*)keys, n_hubs, d_hubs);
    }
    LM_HIP(hipGetLastError());
    return link_launch(d_table, dtype, d_padded, metric, d_adj_out, d_dist_out, d_deg_out, n, cap, e_src, e_dst, e_w, ne, alpha, ws, st);
}

}  // extern "C"
