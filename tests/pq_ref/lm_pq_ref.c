/*
 * lm_pq_ref.c -- CPU restatement of lm_pq_encode and lm_pq_train (include/leann_mi355x.h): the product quantiser's nearest-centroid
 * assignment and its Lloyd iterations.  Test infrastructure: written from the header's contract, shares no code with the kernels
 * (leann_amd/csrc/lm_pq_build_impl.h).
 *
 * The contract, in the words of the header:
 *   x         rows of fp32 with stride ld (an fp16 input is widened by the caller: exact);
 *   chunk j   dimensions [off[j], off[j+1]) -- or [j * d/m, (j+1) * d/m) when off is NULL --; its 256 centroids x len_j floats sit at
 *             float offset 256 * off[j] of the codebooks;
 *   assign    dist_c = acc after { acc = 0.0f; for t: diff = x[lo + t] - cb[c][t]; acc = fmaf(diff, diff, acc); },  c = 0 .. 255;
 *             code = 0, best = +inf; for c ascending: if (dist_c < best) take c.  (Ties: lowest c.  NaN never wins.  Empty chunk: 0.)
 *   update    for every (j, c) with count > 0, every t: sum = 0.0f; for rows v ascending with code[v][j] == c: sum = sum + x[v][lo + t];
 *             cb[c][t] = sum / (float)count.  count == 0: the centroid stays.
 * fp32 throughout; build with -ffp-contract=off.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

static int chunk_lo(const int32_t *off, int32_t d, int32_t m, int j) { return off ? off[j] : j * (d / m); }

static uint8_t nearest(const float *xs, const float *cbj, int len) {
    float best = INFINITY;
    int code = 0;
    for (int c = 0; c < 256; ++c) {
        const float *cen = cbj + (size_t)c * (size_t)len;
        float acc = 0.0f;
        for (int t = 0; t < len; ++t) {
            const float diff = xs[t] - cen[t];
            acc = fmaf(diff, diff, acc);
        }
        if (acc < best) {
            best = acc;
            code = c;
        }
    }
    return (uint8_t)code;
}

static int shape_ok(int64_t n, int32_t ld, int32_t d, int32_t m, const int32_t *off) {
    if (n < 0 || d < 0 || ld < d || m < 1) return 0;
    if (!off) return d % m == 0;
    if (off[0] != 0 || off[m] > d) return 0;
    for (int j = 0; j < m; ++j)
        if (off[j + 1] < off[j]) return 0;
    return 1;
}

int lm_pq_ref_encode(const float *x, int64_t n, int32_t ld, int32_t d, int32_t m, const int32_t *off, const float *cb, uint8_t *codes) {
    if (!shape_ok(n, ld, d, m, off)) return -1;
#pragma omp parallel for schedule(static)
    for (int64_t v = 0; v < n; ++v)
        for (int j = 0; j < m; ++j) {
            const int lo = chunk_lo(off, d, m, j), hi = chunk_lo(off, d, m, j + 1);
            codes[(size_t)v * (size_t)m + (size_t)j] = nearest(x + (size_t)v * (size_t)ld + lo, cb + (size_t)256 * (size_t)lo, hi - lo);
        }
    return 0;
}

int lm_pq_ref_train(const float *x, int64_t s, int32_t ld, int32_t d, int32_t m, const int32_t *off, int32_t iters, float *cb) {
    if (!shape_ok(s, ld, d, m, off) || iters < 0) return -1;
    if (s == 0) return 0;
    int failed = 0;
    /* the chunks are independent of each other through all the iterations */
#pragma omp parallel for schedule(dynamic, 1)
    for (int j = 0; j < m; ++j) {
        const int lo = chunk_lo(off, d, m, j), len = chunk_lo(off, d, m, j + 1) - lo;
        float *cbj = cb + (size_t)256 * (size_t)lo;
        uint8_t *code = (uint8_t *)malloc((size_t)s);
        float *sum = (float *)malloc(sizeof(float) * 256 * (size_t)(len ? len : 1));
        int64_t count[256];
        if (!code || !sum) {
            failed = 1;
            free(code);
            free(sum);
            continue;
        }
        for (int it = 0; it < iters; ++it) {
            for (int64_t v = 0; v < s; ++v) code[v] = nearest(x + (size_t)v * (size_t)ld + lo, cbj, len);
            for (int e = 0; e < 256 * len; ++e) sum[e] = 0.0f;
            memset(count, 0, sizeof(count));
            for (int64_t v = 0; v < s; ++v) { /* rows ascending: each (c, t) sum takes its rows in that order */
                const float *xs = x + (size_t)v * (size_t)ld + lo;
                float *sc = sum + (size_t)code[v] * (size_t)len;
                for (int t = 0; t < len; ++t) sc[t] = sc[t] + xs[t];
                ++count[code[v]];
            }
            for (int c = 0; c < 256; ++c) {
                if (count[c] == 0) continue;
                const float fc = (float)count[c];
                for (int t = 0; t < len; ++t) cbj[(size_t)c * (size_t)len + t] = sum[(size_t)c * (size_t)len + t] / fc;
            }
        }
        free(code);
        free(sum);
    }
    return failed ? -2 : 0;
}
