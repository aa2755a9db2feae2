/*
 * lm_select_ref.c -- CPU restatement of lm_select_neighbors (include/leann_mi355x.h), the select-neighbours heuristic of HNSW
 * construction (Malkov & Yashunin Alg. 4 = faiss shrink_neighbor_list) with Vamana's relaxed second pass (DiskANN occlude_list).
 * Test infrastructure: shares no code with the kernel (leann_amd/csrc/lm_select_impl.h).  The distance function is the oracle's
 * canonical reduction, orc_dist of oracle/lm_oracle.c (this file links against liblm_oracle.so).
 *
 * The rule, in the words of the header:
 *   cand [n][K]  candidate row ids, best first; an id < 0 or >= ntable is an empty slot: never kept, never dereferenced;
 *   dist [n][K]  the candidates' internal distances to their row's base node (squared L2, or -ip; smaller is closer), taken as given;
 *   keep [n][K]  1 = kept.
 *   Strict pass: scan j = 0 .. K-1; skip empty slots; stop keeping once m are kept; keep j unless some already kept i has
 *     dist(cand[j], cand[i]) <= dist[j]  (plain IEEE comparison: NaN never dominates).
 *   Relaxed pass, only when alpha != 1: scan the candidates not yet kept, in order, while fewer than m are kept, with thr[j] in place
 *     of dist[j], tested against everything kept so far; a2 = alpha * alpha in fp32, thr = d / a2 (L2),
 *     thr = -(1.0f - (1.0f + d) / a2) (inner product of unit vectors).
 * fp32 throughout; build with -ffp-contract=off.  `table` is fp32 [ntable][Dp], zero padded (an fp16 table is widened by the caller:
 * exact).
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

float orc_dist(const float *e, const float *q, int32_t Dp, int32_t metric); /* oracle/lm_oracle.c: -ip (metric 0) or squared L2 (1) */

static int dominated_by_kept(const float *table, int32_t Dp, int32_t metric, const int32_t *c, int j, const int *kept, int nkept,
                             float thr) {
    const float *vj = table + (size_t)c[j] * (size_t)Dp;
    for (int t = 0; t < nkept; ++t) {
        const float *vi = table + (size_t)c[kept[t]] * (size_t)Dp;
        if (orc_dist(vj, vi, Dp, metric) <= thr) return 1;
    }
    return 0;
}

int lm_select_ref(const float *table, int64_t ntable, int32_t Dp, int32_t metric, const int32_t *cand, const float *dist, int64_t n,
                  int32_t K, int32_t m, float alpha, uint8_t *keep) {
    if (Dp <= 0 || Dp % 64 || K < 1 || m < 1 || !(alpha >= 1.0f) || n < 0) return -1;
    const float a2 = alpha * alpha;
    int failed = 0;
#pragma omp parallel for schedule(dynamic, 16)
    for (int64_t r = 0; r < n; ++r) {
        const int32_t *c = cand + (size_t)r * (size_t)K;
        const float *d = dist + (size_t)r * (size_t)K;
        uint8_t *kp = keep + (size_t)r * (size_t)K;
        int *kept = (int *)malloc(sizeof(int) * (size_t)K);
        if (!kept) {
            failed = 1;
            continue;
        }
        int nkept = 0;
        memset(kp, 0, (size_t)K);
        /* strict pass */
        for (int j = 0; j < K; ++j) {
            if (c[j] < 0 || (int64_t)c[j] >= ntable) continue;
            if (nkept >= m) break;
            if (dominated_by_kept(table, Dp, metric, c, j, kept, nkept, d[j])) continue;
            kp[j] = 1;
            kept[nkept++] = j;
        }
        /* relaxed pass */
        if (alpha != 1.0f) {
            for (int j = 0; j < K && nkept < m; ++j) {
                if (c[j] < 0 || (int64_t)c[j] >= ntable || kp[j]) continue;
                float thr;
                if (metric == 1) thr = d[j] / a2;
                else thr = -(1.0f - (1.0f + d[j]) / a2);
                if (dominated_by_kept(table, Dp, metric, c, j, kept, nkept, thr)) continue;
                kp[j] = 1;
                kept[nkept++] = j;
            }
        }
        free(kept);
    }
    return failed ? -2 : 0;
}
