// lm_csr_impl.h -- index build time: the finished build's level adjacencies (fixed capacity, lm_graph_level) to the compact CSR that
// lm_index_create_from_csr, csr_format.py and the reference's convert_to_csr.py consume, device to device, and one level of a CSR back
// to the fixed-capacity layout.  Included at the end of lm_search.hip; include/leann_mi355x.h states the contract.
//
// Reference surface replaced: the CSR assembly of convert_to_csr.py:494-548 as leann_amd/gpu_graph_build.py restates it in numpy
// (_assemble_csr: a device-to-host export of every level, two cumulative sums, a scatter over every slot; _with_level0 and the "dense
// array from the CSR" step of prune_preserving_hubs for the way back).
//
// Shape.  Nothing here waits on another workgroup: the two prefix sums are three launches each, and stream order is the only ordering.
//   k_csr_levels_init / k_csr_levels_mark   levels[v] = 1, then one launch per upper level l, ascending: levels[nodes[r]] = l + 1.  Plain
//                      stores: the launches are ordered by the stream, the last writer is the highest level that lists v.
//   k_csr_scan_reduce  one workgroup per tile of CSR_TILE = 1024 items (256 lanes, 4 consecutive items each): the tile's sum;
//   k_csr_scan_parts   ONE workgroup of 1024 lanes walks the tile sums, tile by tile with a carry, and leaves their exclusive prefixes;
//   k_csr_scan_apply   the tiles again: the workgroup's own exclusive scan (wave shuffles, one LDS hand-over) plus the tile's prefix.
//                      Scan A runs over levels[v] + 1 and gives node_offsets; scan B over the per-pointer degrees and gives level_ptr.
//                      B's length, n_level_ptr, is only known on the device: its grids are sized by a bound that is a function of the
//                      arguments (2 ntotal + sum l n_rows[l]) and the kernels read the length from node_offsets[ntotal].
//   k_csr_row_count    a 16-lane group per row at cap <= 64 (four rows per wave, as k_select_neighbors splits them), a wave per row
//                      above: the row's slots are read coalesced, a wave ballot over "slot is a node" gives the degree, which goes to
//                      deg[node_offsets[v] + l] -- the workspace keeps it for _fill.  The level-0 launch comes first and also clears
//                      v's other pointers (the sentinel, levels that do not list v); the upper levels overwrite theirs.
//   k_csr_row_fill     the same split and the same ballot: a survivor goes to level_ptr[node_offsets[v] + l] + popcount(ballot below
//                      my lane), so a wave writes neighbors in ascending address order and nothing is an atomic.
//   k_csr_to_level     the way back, the same split: row r = list `level` of node nodes[r], left-packed, -1 behind it.
// Every index that a kernel forms from device data is checked against the array it goes into before it is used: node ids against
// ntotal, a level against levels[v], a survivor's place against the end of its list (level_ptr[p + 1]), a list against n_neighbors.
#pragma once

namespace lm {

constexpr int CSR_NT = 256;                        // lanes per workgroup of the tile and row kernels
constexpr int CSR_PER = 4;                         // consecutive items per lane of a scan tile
constexpr int CSR_TILE = CSR_NT * CSR_PER;         // items per scan tile: 1024
constexpr int CSR_PARTS_NT = 1024;                 // the one workgroup over the tile sums
constexpr int CSR_GROUP_CAP = 64;                  // up to this cap a row is a 16-lane group's, above it a wave's
constexpr int32_t CSR_MAX_LEVELS = 64;             // LM_CSR_MAX_LEVELS

__device__ __forceinline__ bool csr_is_node(int32_t u, int64_t n) { return (uint32_t)u < (uint32_t)n; }  // n <= INT32_MAX

// the exclusive prefix of x over the workgroup's NT lanes; total = the sum over all of them.  s_wave: NT / 64 words of LDS, free
// again when the call returns.  Every lane of the workgroup calls it.
template <int NT>
__device__ __forceinline__ uint64_t csr_block_scan(uint64_t x, uint64_t* s_wave, uint64_t& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t incl = x;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t up = __shfl_up(incl, d);
        if (lane >= d) incl += up;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    uint64_t below = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) {
        const uint64_t t = s_wave[w];
        below += w < wave ? t : 0;
        total += t;
    }
    __syncthreads();  // s_wave is rewritten by the next call
    return below + incl - x;
}

__global__ __launch_bounds__(CSR_NT) void k_csr_levels_init(int32_t* levels, int64_t n) {
    const int64_t v = (int64_t)blockIdx.x * CSR_NT + threadIdx.x;
    if (v < n) levels[v] = 1;
}

__global__ __launch_bounds__(CSR_NT) void k_csr_levels_mark(const int32_t* nodes, int64_t n_rows, int32_t l, int64_t n, int32_t* levels) {
    const int64_t r = (int64_t)blockIdx.x * CSR_NT + threadIdx.x;
    if (r >= n_rows) return;
    const int64_t v = nodes ? (int64_t)nodes[r] : r;
    if (v >= 0 && v < n) levels[v] = l + 1;
}

// the scans run over in[i] + add, i < n, where n = *d_n when d_n is given (a length that only the device knows) and n_host otherwise
__device__ __forceinline__ int64_t csr_scan_len(const uint64_t* d_n, int64_t n_host) { return d_n ? (int64_t)*d_n : n_host; }

__global__ __launch_bounds__(CSR_NT) void k_csr_scan_reduce(const int32_t* in, int32_t add, const uint64_t* d_n, int64_t n_host, uint64_t* part) {
    __shared__ uint64_t s_wave[CSR_NT / 64];
    const int64_t n = csr_scan_len(d_n, n_host);
    const int64_t i0 = (int64_t)blockIdx.x * CSR_TILE + (int64_t)threadIdx.x * CSR_PER;
    if ((int64_t)blockIdx.x * CSR_TILE >= n) return;  // the grid is sized by a bound: the whole workgroup leaves
    uint64_t sum = 0;
#pragma unroll
    for (int k = 0; k < CSR_PER; ++k)
        if (i0 + k < n) sum += (uint64_t)((int64_t)in[i0 + k] + add);
    uint64_t total;
    csr_block_scan<CSR_NT>(sum, s_wave, total);
    if (threadIdx.x == 0) part[blockIdx.x] = total;
}

// part[b] := the sum of the tiles below b, for the ceil(n / CSR_TILE) tiles; res[0] = n, res[1] = the sum of all items
__global__ __launch_bounds__(CSR_PARTS_NT) void k_csr_scan_parts(uint64_t* part, const uint64_t* d_n, int64_t n_host, uint64_t* res) {
    __shared__ uint64_t s_wave[CSR_PARTS_NT / 64];
    const int64_t n = csr_scan_len(d_n, n_host);
    const int64_t nb = (n + CSR_TILE - 1) / CSR_TILE;
    uint64_t carry = 0;
    for (int64_t base = 0; base < nb; base += CSR_PARTS_NT) {
        const int64_t b = base + threadIdx.x;
        const uint64_t x = b < nb ? part[b] : 0;
        uint64_t total;
        const uint64_t excl = csr_block_scan<CSR_PARTS_NT>(x, s_wave, total);
        if (b < nb) part[b] = carry + excl;
        carry += total;
    }
    if (threadIdx.x == 0) {
        res[0] = (uint64_t)n;
        res[1] = carry;
    }
}

// out[i] = the sum of the items below i, i < n; with_total: out[n] = the sum of all of them as well (then n == 0 still writes out[0] = 0)
__global__ __launch_bounds__(CSR_NT) void k_csr_scan_apply(const int32_t* in, int32_t add, const uint64_t* d_n, int64_t n_host, const uint64_t* part, uint64_t* out,
                                                          int with_total) {
    __shared__ uint64_t s_wave[CSR_NT / 64];
    const int64_t n = csr_scan_len(d_n, n_host);
    if ((int64_t)blockIdx.x * CSR_TILE >= n) {
        if (with_total && n == 0 && blockIdx.x == 0 && threadIdx.x == 0) out[0] = 0;
        return;
    }
    const int64_t i0 = (int64_t)blockIdx.x * CSR_TILE + (int64_t)threadIdx.x * CSR_PER;
    uint64_t x[CSR_PER], sum = 0;
#pragma unroll
    for (int k = 0; k < CSR_PER; ++k) {
        x[k] = i0 + k < n ? (uint64_t)((int64_t)in[i0 + k] + add) : 0;
        sum += x[k];
    }
    uint64_t total;
    uint64_t run = part[blockIdx.x] + csr_block_scan<CSR_NT>(sum, s_wave, total);
#pragma unroll
    for (int k = 0; k < CSR_PER; ++k) {
        if (i0 + k < n) {
            out[i0 + k] = run;
            run += x[k];
            if (with_total && i0 + k == n - 1) out[n] = run;
        }
    }
}

// Who I am in a row kernel: G lanes per row (64: a wave, 16: a quarter of one), CSR_NT / G rows per workgroup.
template <bool WAVE>
struct CsrRowLane {
    static constexpr int G = WAVE ? 64 : 16;
    int sub;      // my lane within the row's group
    int shift;    // where the group's bits start in the wave's ballot
    int64_t r;    // the row
    __device__ __forceinline__ CsrRowLane() {
        sub = threadIdx.x % G;
        shift = WAVE ? 0 : (threadIdx.x & 63) / G * G;
        r = (int64_t)blockIdx.x * (CSR_NT / G) + threadIdx.x / G;
    }
    // the group's part of a wave ballot (every lane of the wave calls this): cnt = the group's lanes with ok, below = those under mine
    __device__ __forceinline__ void ballot(bool ok, int& cnt, int& below) const {
        unsigned long long m = __ballot(ok);
        if (!WAVE) m = (m >> shift) & 0xffffull;
        cnt = __popcll(m);
        below = __popcll(m & ((1ull << sub) - 1ull));
    }
};

// deg[off[v] + l] = the number of slots of v's row that hold a node.  The level-0 launch (l == 0) also clears the other pointers of v.
template <bool WAVE>
__global__ __launch_bounds__(CSR_NT) void k_csr_row_count(const int32_t* adj, const int32_t* nodes, int64_t n_rows, int cap, int32_t l, int64_t n, const int32_t* levels,
                                                         const uint64_t* off, int32_t* deg) {
    const CsrRowLane<WAVE> me;
    constexpr int G = CsrRowLane<WAVE>::G;
    bool live = me.r < n_rows;
    const int64_t v = live ? (nodes ? (int64_t)nodes[me.r] : me.r) : -1;
    live = live && v >= 0 && v < n;
    const int32_t nl = live ? levels[v] : 0;
    live = live && l < nl;  // (always, after the mark launches of the same arrays)
    const int32_t* row = adj + me.r * cap;
    int degree = 0;
    for (int c0 = 0; c0 < cap; c0 += G) {  // cap is the same in every lane: so is the number of ballots
        const int c = c0 + me.sub;
        int cnt, below;
        me.ballot(live && c < cap && csr_is_node(row[c], n), cnt, below);
        degree += cnt;
    }
    if (!live) return;
    const int64_t p = (int64_t)off[v] + l;
    if (me.sub == 0) deg[p] = degree;
    if (l == 0)
        for (int j = 1 + me.sub; j <= nl; j += G) deg[p + j] = 0;  // v has nl + 1 pointers; the last one, the sentinel, never gets a list
}

template <bool WAVE>
__global__ __launch_bounds__(CSR_NT) void k_csr_row_fill(const int32_t* adj, const int32_t* nodes, int64_t n_rows, int cap, int32_t l, int64_t n, const int32_t* levels,
                                                        const uint64_t* off, const uint64_t* level_ptr, int32_t* neighbors) {
    const CsrRowLane<WAVE> me;
    constexpr int G = CsrRowLane<WAVE>::G;
    bool live = me.r < n_rows;
    const int64_t v = live ? (nodes ? (int64_t)nodes[me.r] : me.r) : -1;
    live = live && v >= 0 && v < n;
    live = live && l < levels[live ? v : 0];
    uint64_t at = 0, end = 0;
    if (live) {
        const int64_t p = (int64_t)off[v] + l;  // p + 1 is at most v's sentinel
        at = level_ptr[p];
        end = level_ptr[p + 1];
    }
    const int32_t* row = adj + me.r * cap;
    for (int c0 = 0; c0 < cap; c0 += G) {
        const int c = c0 + me.sub;
        const int32_t u = live && c < cap ? row[c] : -1;
        const bool ok = live && csr_is_node(u, n);
        int cnt, below;
        me.ballot(ok, cnt, below);
        if (ok && at + below < end) neighbors[at + below] = u;  // (at + below < end: always, on the arrays _count saw)
        at += cnt;
    }
}

template <bool WAVE>
__global__ __launch_bounds__(CSR_NT) void k_csr_to_level(int64_t n, const uint64_t* off, const uint64_t* level_ptr, int64_t n_level_ptr, const int32_t* neighbors,
                                                        int64_t n_neighbors, const int32_t* levels, int32_t level, const int32_t* nodes, int64_t n_rows, int cap,
                                                        int32_t* adj, int32_t* deg, unsigned long long* overflow) {
    const CsrRowLane<WAVE> me;
    constexpr int G = CsrRowLane<WAVE>::G;
    if (me.r >= n_rows) return;
    const int64_t v = nodes ? (int64_t)nodes[me.r] : me.r;
    uint64_t b = 0, e = 0;
    if (v >= 0 && v < n && level < levels[v]) {
        const uint64_t p = off[v] + (uint64_t)level;
        if (p + 1 < (uint64_t)n_level_ptr) {
            b = level_ptr[p];
            e = level_ptr[p + 1];
        }
        if (b > e || e > (uint64_t)n_neighbors) b = e = 0;  // not a CSR: an empty row, nothing is dereferenced
    }
    const uint64_t len = e - b;
    const int keep = (int)(len < (uint64_t)cap ? len : (uint64_t)cap);
    int32_t* row = adj + me.r * cap;
    for (int c = me.sub; c < cap; c += G) row[c] = c < keep ? neighbors[b + c] : -1;
    if (me.sub == 0) {
        if (deg) deg[me.r] = keep;
        if (overflow && len > (uint64_t)cap) atomicAdd(overflow, (unsigned long long)(len - cap));
    }
}

inline size_t csr_align(size_t b) { return (b + 255) & ~(size_t)255; }

// what the forward calls reject alike; max_ptr = the bound on n_level_ptr that sizes the workspace and the grids of scan B: v has
// top(v) + 2 pointers, and a node has top >= l only if one of the levels l.. lists it, so n_level_ptr <= 2 ntotal + sum l * n_rows[l]
inline int csr_check_levels(int64_t ntotal, const lm_graph_level* levels, int32_t n_levels, int64_t* max_ptr) {
    if (!levels) LM_FAIL(LM_EINVAL, "levels is NULL");
    if (n_levels < 1 || n_levels > CSR_MAX_LEVELS) LM_FAIL(LM_EINVAL, "n_levels must be in [1, LM_CSR_MAX_LEVELS = " + std::to_string(CSR_MAX_LEVELS) + "]");
    if (ntotal < 0 || ntotal > 0x7fffffffll) LM_FAIL(LM_EINVAL, "ntotal must be in [0, INT32_MAX]");
    int64_t mp = 2 * ntotal;
    for (int32_t l = 0; l < n_levels; ++l) {
        const lm_graph_level& L = levels[l];
        const std::string at = "levels[" + std::to_string(l) + "]: ";
        if (L.cap < 1) LM_FAIL(LM_EINVAL, at + "cap must be at least 1");
        if (L.n_rows < 0 || L.n_rows > ntotal) LM_FAIL(LM_EINVAL, at + "n_rows must be in [0, ntotal]");
        if (l == 0 && (L.d_nodes || L.n_rows != ntotal)) LM_FAIL(LM_EINVAL, "levels[0] must be the identity level: d_nodes NULL and n_rows == ntotal");
        if (l > 0 && L.n_rows > 0 && !L.d_nodes && L.n_rows != ntotal) LM_FAIL(LM_EINVAL, at + "d_nodes is NULL but n_rows != ntotal");
        if (L.n_rows > 0 && !L.d_adj) LM_FAIL(LM_EINVAL, at + "d_adj is NULL");
        mp += (int64_t)l * L.n_rows;
    }
    *max_ptr = mp;
    return LM_OK;
}

// the workspace: the two results, the tile sums of scan A and of scan B, the per-pointer degrees
struct CsrWorkspace {
    uint64_t *res, *part_a, *part_b;
    int32_t* deg;
    int64_t nb_a, nb_b;
    size_t bytes;
    CsrWorkspace(void* ws, int64_t ntotal, int64_t max_ptr) {
        nb_a = (ntotal + CSR_TILE - 1) / CSR_TILE;
        nb_b = (max_ptr + CSR_TILE - 1) / CSR_TILE;
        char* p = (char*)ws;
        size_t o = 0;
        res = (uint64_t*)(p + o);
        o += csr_align(4 * 8);
        part_a = (uint64_t*)(p + o);
        o += csr_align((size_t)nb_a * 8);
        part_b = (uint64_t*)(p + o);
        o += csr_align((size_t)nb_b * 8);
        deg = (int32_t*)(p + o);
        o += csr_align((size_t)max_ptr * 4);
        bytes = o;
    }
};

inline int csr_check_workspace(const CsrWorkspace& w, const void* d_workspace, size_t workspace_bytes) {
    if (!d_workspace) LM_FAIL(LM_EINVAL, "d_workspace is NULL");
    if ((uintptr_t)d_workspace % 8) LM_FAIL(LM_EINVAL, "d_workspace must be 8-byte aligned");
    if (workspace_bytes < w.bytes) LM_FAIL(LM_EINVAL, "workspace smaller than lm_graph_levels_to_csr_workspace_bytes(ntotal, levels, n_levels)");
    return LM_OK;
}

// one launch of a row kernel per level, in level order: the group form up to CSR_GROUP_CAP, the wave form above
#define LM_CSR_ROWS(kernel, L, ...)                                                                                           \
    do {                                                                                                                      \
        if ((L).cap <= CSR_GROUP_CAP)                                                                                         \
            hipLaunchKernelGGL((kernel<false>), dim3((unsigned)(((L).n_rows + CSR_NT / 16 - 1) / (CSR_NT / 16))), dim3(CSR_NT), 0, st, __VA_ARGS__); \
        else                                                                                                                  \
            hipLaunchKernelGGL((kernel<true>), dim3((unsigned)(((L).n_rows + CSR_NT / 64 - 1) / (CSR_NT / 64))), dim3(CSR_NT), 0, st, __VA_ARGS__);  \
    } while (0)

}  // namespace lm

extern "C" {

size_t lm_graph_levels_to_csr_workspace_bytes(int64_t ntotal, const lm_graph_level* levels, int32_t n_levels) {
    int64_t max_ptr = 0;
    if (lm::csr_check_levels(ntotal, levels, n_levels, &max_ptr) != LM_OK || ntotal == 0) return 0;
    return lm::CsrWorkspace(nullptr, ntotal, max_ptr).bytes;
}

int lm_graph_levels_to_csr_count(int64_t ntotal, const lm_graph_level* levels, int32_t n_levels, int32_t* d_levels, uint64_t* d_node_offsets, void* d_workspace,
                                 size_t workspace_bytes, int64_t* n_level_ptr, int64_t* n_neighbors, void* stream) {
    using namespace lm;
    int64_t max_ptr = 0;
    if (int rc = csr_check_levels(ntotal, levels, n_levels, &max_ptr)) return rc;
    if (!d_node_offsets || !n_level_ptr || !n_neighbors) LM_FAIL(LM_EINVAL, "NULL buffer");
    hipStream_t st = (hipStream_t)stream;
    if (ntotal == 0) {
        hipLaunchKernelGGL(k_csr_scan_apply, dim3(1), dim3(CSR_NT), 0, st, (const int32_t*)nullptr, 1, (const uint64_t*)nullptr, (int64_t)0, (const uint64_t*)nullptr,
                           d_node_offsets, 1);
        LM_HIP(hipGetLastError());
        *n_level_ptr = *n_neighbors = 0;
        return LM_OK;
    }
    if (!d_levels) LM_FAIL(LM_EINVAL, "NULL buffer");
    const CsrWorkspace w(d_workspace, ntotal, max_ptr);
    if (int rc = csr_check_workspace(w, d_workspace, workspace_bytes)) return rc;
    const int64_t n = ntotal;
    const uint64_t* d_nptr = d_node_offsets + n;  // n_level_ptr, once scan A has run
    // top levels
    hipLaunchKernelGGL(k_csr_levels_init, dim3((unsigned)((n + CSR_NT - 1) / CSR_NT)), dim3(CSR_NT), 0, st, d_levels, n);
    for (int32_t l = 1; l < n_levels; ++l)
        if (levels[l].n_rows > 0)
            hipLaunchKernelGGL(k_csr_levels_mark, dim3((unsigned)((levels[l].n_rows + CSR_NT - 1) / CSR_NT)), dim3(CSR_NT), 0, st, levels[l].d_nodes, levels[l].n_rows, l, n,
                               d_levels);
    // scan A: node_offsets
    hipLaunchKernelGGL(k_csr_scan_reduce, dim3((unsigned)w.nb_a), dim3(CSR_NT), 0, st, (const int32_t*)d_levels, 1, (const uint64_t*)nullptr, n, w.part_a);
    hipLaunchKernelGGL(k_csr_scan_parts, dim3(1), dim3(CSR_PARTS_NT), 0, st, w.part_a, (const uint64_t*)nullptr, n, w.res + 2);
    hipLaunchKernelGGL(k_csr_scan_apply, dim3((unsigned)w.nb_a), dim3(CSR_NT), 0, st, (const int32_t*)d_levels, 1, (const uint64_t*)nullptr, n, (const uint64_t*)w.part_a,
                       d_node_offsets, 1);
    // degrees, level 0 first (it clears what the upper levels do not write)
    for (int32_t l = 0; l < n_levels; ++l)
        if (levels[l].n_rows > 0)
            LM_CSR_ROWS(k_csr_row_count, levels[l], levels[l].d_adj, levels[l].d_nodes, levels[l].n_rows, (int)levels[l].cap, l, n, (const int32_t*)d_levels,
                        (const uint64_t*)d_node_offsets, w.deg);
    // scan B up to the tile prefixes: its total is n_neighbors
    hipLaunchKernelGGL(k_csr_scan_reduce, dim3((unsigned)w.nb_b), dim3(CSR_NT), 0, st, (const int32_t*)w.deg, 0, d_nptr, (int64_t)0, w.part_b);
    hipLaunchKernelGGL(k_csr_scan_parts, dim3(1), dim3(CSR_PARTS_NT), 0, st, w.part_b, d_nptr, (int64_t)0, w.res);
    LM_HIP(hipGetLastError());
    uint64_t h[2] = {0, 0};
    LM_HIP(hipMemcpyAsync(h, w.res, sizeof(h), hipMemcpyDeviceToHost, st));
    LM_HIP(hipStreamSynchronize(st));  // the one synchronisation: the caller sizes level_ptr and neighbors by these
    *n_level_ptr = (int64_t)h[0];
    *n_neighbors = (int64_t)h[1];
    return LM_OK;
}

int lm_graph_levels_to_csr_fill(int64_t ntotal, const lm_graph_level* levels, int32_t n_levels, const int32_t* d_levels, const uint64_t* d_node_offsets,
                                uint64_t* d_level_ptr, int32_t* d_neighbors, void* d_workspace, size_t workspace_bytes, void* stream) {
    using namespace lm;
    int64_t max_ptr = 0;
    if (int rc = csr_check_levels(ntotal, levels, n_levels, &max_ptr)) return rc;
    if (ntotal == 0) return LM_OK;
    if (!d_levels || !d_node_offsets || !d_level_ptr || !d_neighbors) LM_FAIL(LM_EINVAL, "NULL buffer");
    const CsrWorkspace w(d_workspace, ntotal, max_ptr);
    if (int rc = csr_check_workspace(w, d_workspace, workspace_bytes)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = ntotal;
    hipLaunchKernelGGL(k_csr_scan_apply, dim3((unsigned)w.nb_b), dim3(CSR_NT), 0, st, (const int32_t*)w.deg, 0, d_node_offsets + n, (int64_t)0, (const uint64_t*)w.part_b,
                       d_level_ptr, 0);
    for (int32_t l = 0; l < n_levels; ++l)
        if (levels[l].n_rows > 0)
            LM_CSR_ROWS(k_csr_row_fill, levels[l], levels[l].d_adj, levels[l].d_nodes, levels[l].n_rows, (int)levels[l].cap, l, n, d_levels, d_node_offsets,
                        (const uint64_t*)d_level_ptr, d_neighbors);
    LM_HIP(hipGetLastError());
    return LM_OK;
}

int lm_graph_csr_to_level(int64_t ntotal, const uint64_t* d_node_offsets, const uint64_t* d_level_ptr, int64_t n_level_ptr, const int32_t* d_neighbors,
                          int64_t n_neighbors, const int32_t* d_levels, int32_t level, const int32_t* d_nodes, int64_t n_rows, int32_t cap, int32_t* d_adj,
                          int32_t* d_deg, int64_t* d_overflow, void* stream) {
    using namespace lm;
    if (ntotal < 0 || ntotal > 0x7fffffffll) LM_FAIL(LM_EINVAL, "ntotal must be in [0, INT32_MAX]");
    if (n_level_ptr < 0 || n_neighbors < 0) LM_FAIL(LM_EINVAL, "n_level_ptr / n_neighbors must not be negative");
    if (level < 0) LM_FAIL(LM_EINVAL, "level must not be negative");
    if (cap < 1) LM_FAIL(LM_EINVAL, "cap must be at least 1");
    if (n_rows < 0 || n_rows > ntotal) LM_FAIL(LM_EINVAL, "n_rows must be in [0, ntotal]");
    if (!d_nodes && n_rows != ntotal) LM_FAIL(LM_EINVAL, "d_nodes is NULL (the identity) but n_rows != ntotal");
    if (n_rows == 0) return LM_OK;
    if (!d_node_offsets || !d_levels || !d_adj || (n_level_ptr > 0 && !d_level_ptr) || (n_neighbors > 0 && !d_neighbors)) LM_FAIL(LM_EINVAL, "NULL buffer");
    hipStream_t st = (hipStream_t)stream;
    struct { int64_t n_rows; int32_t cap; } L = {n_rows, cap};
    LM_CSR_ROWS(k_csr_to_level, L, ntotal, d_node_offsets, d_level_ptr, n_level_ptr, d_neighbors, n_neighbors, d_levels, level, d_nodes, n_rows, (int)cap, d_adj, d_deg,
                (unsigned long long*)d_overflow);
    LM_HIP(hipGetLastError());
    return LM_OK;
}

}  // extern "C"
