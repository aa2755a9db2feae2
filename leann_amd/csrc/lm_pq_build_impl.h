// lm_pq_build_impl.h -- index build time: the product quantiser's two steps as kernels -- nearest-centroid assignment (lm_pq_encode) and
// Lloyd iterations over a sample (lm_pq_train).  Included at the end of lm_search.hip.  What they produce is what lm_pq_attach /
// lm_pq_attach_chunked take: chunk j = 256 centroids x len_j floats at float offset 256 * chunk_offsets[j] (uniform: [m][256][d/m]).
//
// Reference surface replaced: leann_amd/pq.py's torch forms train_pq / encode_pq (the role of DiskANN's generate_pq_pivots /
// generate_pq_data_from_pivots behind diskann_backend.py:105-111), which stay the default.
//
// THE CONTRACT IS THE ARITHMETIC (tests/pq_ref/lm_pq_ref.c restates it; include/leann_mi355x.h words it for the caller):
//   assignment, chunk j = dimensions [lo, lo + len) of row v, always squared L2 whatever the index metric:
//     dist_c = acc after  acc = 0.0f; for t in 0..len-1: diff = x[lo + t] - cb[c][t]; acc = fmaf(diff, diff, acc)       (c = 0..255)
//     -- oracle/lm_oracle_pq.c:orc_pq_lut's L2 form with the row as the query; fp16 rows are widened first (exact) --
//     code = 0, best = +inf; for c ascending: if (dist_c < best) { best = dist_c; code = c; }
//     (ties go to the lowest c, a NaN distance never wins, an all-NaN or zero-length chunk gets code 0);
//   update, after each assignment, for every (j, c) with count > 0 and every coordinate t:
//     sum = 0.0f; for rows v ASCENDING with code[v][j] == c: sum = sum + x[v][lo + t];   cb[c][t] = sum / (float)count
//     (IEEE fp32, no contraction; count == 0 leaves the centroid as it was).  No floating-point atomics anywhere: the trained
//     codebooks are a function of the input bits alone.
//
// Shape.  k_pq_assign: one workgroup = 256 * R rows x one chunk; the chunk's 256 centroids are staged in LDS (<= 64 KB at
// LM_PQ_MAX_SUB) and read back as broadcasts -- every lane reads the same address --, each thread keeps R rows' chunk in registers,
// so one LDS read feeds R rows.  Chunk lengths 2, 4, 8, 16 and 32 are compiled with the length as a constant; every other length
// runs the same code with registers for LM_PQ_MAX_SUB coordinates and a run-time bound.  k_pq_update: one workgroup per chunk, one
// thread per centroid; the workgroup walks the sample in row order through LDS tiles (the chunk's code column, which the training
// assignment wrote chunk-major so that the column is contiguous, and the rows' coordinates), and every thread adds the rows that
// carry its centroid to len registers -- ascending rows by construction, no sort, no atomics.
#pragma once

#include <climits>

namespace lm {

constexpr int PQB_CAP = LM_PQ_MAX_SUB;

template <bool F16>
__device__ __forceinline__ float pqb_load(const void* x, int64_t off) {
    if constexpr (F16) return __half2float(((const __half*)x)[off]);
    else return ((const float*)x)[off];
}

// LEN > 0: every chunk of the launch has that length; LEN == 0: run-time `len` (0 .. PQB_CAP).
// Chunks j0 .. j0 + nj - 1, all `len` long, the first at dimension lo0; blockIdx.x = tile * nj + (j - j0).
// codes[v * code_rs + j * code_cs]: (m, 1) = the ABI's [n][m]; (1, s) = the training workspace's chunk-major [m][s].
template <int LEN, int R, bool F16>
__global__ __launch_bounds__(256) void k_pq_assign(const void* x, int64_t n, int ld, int j0, int lo0, int len, int nj, const float* cb,
                                                   uint8_t* codes, int64_t code_rs, int64_t code_cs) {
    constexpr int CAP = LEN ? LEN : PQB_CAP;
    __shared__ __align__(16) float s_cb[256 * CAP];
    const int L = LEN ? LEN : len;
    const int tid = threadIdx.x;
    const int jj = (int)(blockIdx.x % (unsigned)nj);
    const int64_t tile = blockIdx.x / (unsigned)nj;
    const int j = j0 + jj, lo = lo0 + jj * L;
    const float* cbj = cb + (size_t)256 * lo;
    for (int e = tid; e < 256 * L; e += 256) s_cb[e] = cbj[e];
    float xr[R][CAP];
    int64_t row[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        row[r] = tile * (256 * R) + r * 256 + tid;
#pragma unroll
        for (int t = 0; t < CAP; ++t) {
            if (LEN || t < L) xr[r][t] = row[r] < n ? pqb_load<F16>(x, row[r] * ld + lo + t) : 0.0f;
        }
    }
    __syncthreads();
    float best[R];
    int code[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        best[r] = __builtin_inff();
        code[r] = 0;
    }
#pragma unroll 2
    for (int c = 0; c < 256; ++c) {
        const float* cc = s_cb + c * L;
        float acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = 0.0f;
#pragma unroll
        for (int t = 0; t < CAP; ++t) {
            if (LEN || t < L) {  // (wave-uniform)
                const float cv = cc[t];
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const float diff = xr[r][t] - cv;
                    acc[r] = __builtin_fmaf(diff, diff, acc[r]);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (acc[r] < best[r]) {
                best[r] = acc[r];
                code[r] = c;
            }
    }
#pragma unroll
    for (int r = 0; r < R; ++r)
        if (row[r] < n) codes[row[r] * code_rs + (int64_t)j * code_cs] = (uint8_t)code[r];
}

// One workgroup per chunk (blockIdx.x = j - j0), thread c = centroid c.  colcodes: the workspace's [m][s] bytes.
template <int LEN, bool F16>
__global__ __launch_bounds__(256) void k_pq_update(const void* x, int64_t s, int ld, int j0, int lo0, int len, const uint8_t* colcodes, float* cb) {
    constexpr int CAP = LEN ? LEN : PQB_CAP;
    constexpr int T = LEN ? 256 : 128;  // rows per LDS tile
    __shared__ __align__(16) float s_x[T * CAP];
    __shared__ __align__(16) uint32_t s_code[T];
    const int L = LEN ? LEN : len;
    const int c = threadIdx.x;
    const int j = j0 + (int)blockIdx.x, lo = lo0 + (int)blockIdx.x * L;
    const uint8_t* col = colcodes + (size_t)j * (size_t)s;
    float sum[CAP];
#pragma unroll
    for (int t = 0; t < CAP; ++t) sum[t] = 0.0f;
    int count = 0;
    for (int64_t v0 = 0; v0 < s; v0 += T) {
        if (c < T) {
            const int64_t v = v0 + c;
            s_code[c] = v < s ? (uint32_t)col[v] : 0xFFFFFFFFu;  // no centroid: a row past the end
#pragma unroll
            for (int t = 0; t < CAP; ++t) {
                if (LEN || t < L) s_x[c * L + t] = v < s ? pqb_load<F16>(x, v * ld + lo + t) : 0.0f;
            }
        }
        __syncthreads();
        for (int i = 0; i < T; i += 4) {
            const uint4 w = *(const uint4*)(s_code + i);
            const uint32_t cw[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (cw[k] == (uint32_t)c) {
                    ++count;
                    const float* xv = s_x + (i + k) * L;
#pragma unroll
                    for (int t = 0; t < CAP; ++t) {
                        if (LEN || t < L) sum[t] = sum[t] + xv[t];
                    }
                }
        }
        __syncthreads();
    }
    if (count > 0) {
        float* out = cb + (size_t)256 * lo + (size_t)c * L;
        const float fc = (float)count;
#pragma unroll
        for (int t = 0; t < CAP; ++t) {
            if (LEN || t < L) out[t] = sum[t] / fc;
        }
    }
}

struct PqbRun {  // consecutive chunks of one length
    int j0, lo0, len, nj;
};

// The envelope both entry points share; fills `runs`.  Returns LM_OK or LM_EINVAL (message set).
static int pqb_validate(int32_t dtype, int64_t n, int32_t ld, int32_t d, int32_t m, const int32_t* chunk_offsets, std::vector<PqbRun>& runs) {
    if (dtype != LM_DTYPE_F32 && dtype != LM_DTYPE_F16) LM_FAIL(LM_EINVAL, "dtype must be f32 or f16");
    if (n < 0) LM_FAIL(LM_EINVAL, "the row count must not be negative");
    if (d < 0 || ld < d) LM_FAIL(LM_EINVAL, "ld must be >= d >= 0");
    if (m < 1 || m > 4096) LM_FAIL(LM_EINVAL, "m must be in [1, 4096]");
    if (!chunk_offsets) {
        if (d % m) LM_FAIL(LM_EINVAL, "uniform layout: m must divide d");
        if (d / m > LM_PQ_MAX_SUB) LM_FAIL(LM_EINVAL, "chunk longer than LM_PQ_MAX_SUB = " + std::to_string(LM_PQ_MAX_SUB));
        runs.push_back({0, 0, d / m, m});
        return LM_OK;
    }
    if (chunk_offsets[0] != 0) LM_FAIL(LM_EINVAL, "chunk_offsets[0] must be 0");
    for (int j = 0; j < m; ++j) {
        const int64_t len = (int64_t)chunk_offsets[j + 1] - chunk_offsets[j];
        if (len < 0) LM_FAIL(LM_EINVAL, "chunk_offsets must not decrease");
        if (len > LM_PQ_MAX_SUB) LM_FAIL(LM_EINVAL, "chunk longer than LM_PQ_MAX_SUB = " + std::to_string(LM_PQ_MAX_SUB));
    }
    if (chunk_offsets[m] > d) LM_FAIL(LM_EINVAL, "chunk_offsets[m] must be <= d");
    for (int j = 0; j < m; ++j) {
        const int len = chunk_offsets[j + 1] - chunk_offsets[j];
        if (!runs.empty() && runs.back().len == len) ++runs.back().nj;
        else runs.push_back({j, chunk_offsets[j], len, 1});
    }
    return LM_OK;
}

template <int LEN, int R>
static int pqb_assign_launch(const PqbRun& r, bool f16, const void* x, int64_t n, int ld, const float* cb, uint8_t* codes, int64_t rs, int64_t cs,
                             hipStream_t st) {
    const int64_t blocks = (n + 256 * R - 1) / (256 * R) * r.nj;
    if (blocks > INT_MAX) LM_FAIL(LM_EINVAL, "too many rows for one launch");
    dim3 grid((unsigned)blocks), block(256);
    if (f16) hipLaunchKernelGGL((k_pq_assign<LEN, R, true>), grid, block, 0, st, x, n, ld, r.j0, r.lo0, r.len, r.nj, cb, codes, rs, cs);
    else hipLaunchKernelGGL((k_pq_assign<LEN, R, false>), grid, block, 0, st, x, n, ld, r.j0, r.lo0, r.len, r.nj, cb, codes, rs, cs);
    return LM_OK;
}

static int pqb_assign(const std::vector<PqbRun>& runs, bool f16, const void* x, int64_t n, int ld, const float* cb, uint8_t* codes, int64_t rs,
                      int64_t cs, hipStream_t st) {
    for (const PqbRun& r : runs) {
        int rc;
        switch (r.len) {
            case 2: rc = pqb_assign_launch<2, 4>(r, f16, x, n, ld, cb, codes, rs, cs, st); break;
            case 4: rc = pqb_assign_launch<4, 4>(r, f16, x, n, ld, cb, codes, rs, cs, st); break;
            case 8: rc = pqb_assign_launch<8, 4>(r, f16, x, n, ld, cb, codes, rs, cs, st); break;
            case 16: rc = pqb_assign_launch<16, 2>(r, f16, x, n, ld, cb, codes, rs, cs, st); break;
            case 32: rc = pqb_assign_launch<32, 1>(r, f16, x, n, ld, cb, codes, rs, cs, st); break;
            default: rc = pqb_assign_launch<0, 1>(r, f16, x, n, ld, cb, codes, rs, cs, st); break;
        }
        if (rc) return rc;
    }
    LM_HIP(hipGetLastError());
    return LM_OK;
}

template <int LEN>
static void pqb_update_launch(const PqbRun& r, bool f16, const void* x, int64_t s, int ld, const uint8_t* colcodes, float* cb, hipStream_t st) {
    dim3 grid((unsigned)r.nj), block(256);
    if (f16) hipLaunchKernelGGL((k_pq_update<LEN, true>), grid, block, 0, st, x, s, ld, r.j0, r.lo0, r.len, colcodes, cb);
    else hipLaunchKernelGGL((k_pq_update<LEN, false>), grid, block, 0, st, x, s, ld, r.j0, r.lo0, r.len, colcodes, cb);
}

static int pqb_update(const std::vector<PqbRun>& runs, bool f16, const void* x, int64_t s, int ld, const uint8_t* colcodes, float* cb, hipStream_t st) {
    for (const PqbRun& r : runs) {
        switch (r.len) {
            case 0: break;  // a zero-length chunk has no coordinates
            case 2: pqb_update_launch<2>(r, f16, x, s, ld, colcodes, cb, st); break;
            case 4: pqb_update_launch<4>(r, f16, x, s, ld, colcodes, cb, st); break;
            case 8: pqb_update_launch<8>(r, f16, x, s, ld, colcodes, cb, st); break;
            case 16: pqb_update_launch<16>(r, f16, x, s, ld, colcodes, cb, st); break;
            case 32: pqb_update_launch<32>(r, f16, x, s, ld, colcodes, cb, st); break;
            default: pqb_update_launch<0>(r, f16, x, s, ld, colcodes, cb, st); break;
        }
    }
    LM_HIP(hipGetLastError());
    return LM_OK;
}

}  // namespace lm

extern "C" {

int lm_pq_encode(const void* d_x, int32_t dtype, int64_t n, int32_t ld, int32_t d, int32_t m, const int32_t* chunk_offsets, const float* d_codebooks,
                 uint8_t* d_codes, void* stream) {
    std::vector<lm::PqbRun> runs;
    if (int rc = lm::pqb_validate(dtype, n, ld, d, m, chunk_offsets, runs)) return rc;
    if (n == 0) return LM_OK;
    if (!d_x || !d_codebooks || !d_codes) LM_FAIL(LM_EINVAL, "NULL buffer");
    if ((n + 255) / 256 * m > INT_MAX) LM_FAIL(LM_EINVAL, "too many rows for one launch");
    return lm::pqb_assign(runs, dtype == LM_DTYPE_F16, d_x, n, ld, d_codebooks, d_codes, m, 1, (hipStream_t)stream);
}

size_t lm_pq_train_workspace_bytes(int64_t s, int32_t d, int32_t m) {
    (void)d;
    if (s <= 0 || m < 1) return 0;
    return ((size_t)s * (size_t)m + 255) / 256 * 256;  // the sample's codes, chunk-major [m][s]
}

int lm_pq_train(const void* d_x, int32_t dtype, int64_t s, int32_t ld, int32_t d, int32_t m, const int32_t* chunk_offsets, int32_t iters,
                float* d_codebooks, void* d_workspace, size_t workspace_bytes, void* stream) {
    std::vector<lm::PqbRun> runs;
    if (int rc = lm::pqb_validate(dtype, s, ld, d, m, chunk_offsets, runs)) return rc;
    if (iters < 0) LM_FAIL(LM_EINVAL, "iters must not be negative");
    if (s == 0 || iters == 0) return LM_OK;
    if (!d_x || !d_codebooks || !d_workspace) LM_FAIL(LM_EINVAL, "NULL buffer");
    if (workspace_bytes < lm_pq_train_workspace_bytes(s, d, m)) LM_FAIL(LM_EINVAL, "workspace smaller than lm_pq_train_workspace_bytes(s, d, m)");
    if (s > INT_MAX || (s + 255) / 256 * m > INT_MAX) LM_FAIL(LM_EINVAL, "sample too large (a centroid's row count is a 32-bit integer)");
    const bool f16 = dtype == LM_DTYPE_F16;
    hipStream_t st = (hipStream_t)stream;
    uint8_t* colcodes = (uint8_t*)d_workspace;
    for (int it = 0; it < iters; ++it) {
        if (int rc = lm::pqb_assign(runs, f16, d_x, s, ld, d_codebooks, colcodes, 1, s, st)) return rc;
        if (int rc = lm::pqb_update(runs, f16, d_x, s, ld, colcodes, d_codebooks, st)) return rc;
    }
    return LM_OK;
}

}  // extern "C"
