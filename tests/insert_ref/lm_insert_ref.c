/*
 * lm_insert_ref.c -- CPU restatement of lm_graph_insert_batch (include/leann_mi355x.h): one insert step of the batched HNSW builder.
 * Test infrastructure: shares no code with the kernels (leann_amd/csrc/lm_insert_impl.h).  Steps 1 and 3-8 are restated here.  Step 2,
 * the search, is an INPUT: S is what lm_index_search_device returned on the view for the queries of step 1 (the header says the insert's
 * search is that call, and the view tests pin it to the oracle).  Step 6 is the unchanged tests/select_ref/lm_select_ref.c and step 9 the
 * unchanged tests/link_ref/lm_link_ref.c, compiled into the same object and called once each.
 *
 * The rules, in the words of the header:
 *   1. the query of row i is the first d values of table row v = batch[i]; v outside [0, n): VOID, all zeros, all candidates empty, only
 *      invalid edges, nothing cleared;
 *   3. replace == 0: the kk entries of S(i) in the order returned;
 *   4. replace == 1: S(i) with the entries whose label is v made empty, then the cap slots of row v in slot order (a value outside
 *      [0, n) is empty); the first occurrence of an id survives; the non-empty entries ordered by (internal distance ascending, position
 *      ascending), -0 counting as +0; empties last;
 *   5. an entry whose internal distance is not finite is empty -- in step 4 after the dedupe, before the ordering --; empty = (-1, +inf);
 *   6. keep = lm_select_ref(cand, dist, K, m, alpha);
 *   7. edge i m + r = v -> u, edge b m + i m + r = u -> v for the r-th kept candidate (u, w) of row i; every other edge (-1, -1);
 *   8. replace == 1: every non-void row v := empty, after all candidates are formed;
 *   9. lm_link_ref ONCE with the 2 b m edges.
 * `table` is fp32 [n][Dp], zero padded (an fp16 table is widened by the caller: exact).  s_dist is what the search DECODED: squared L2, or
 * +ip; the internal distance is its exact negation for the inner product.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

int lm_select_ref(const float *table, int64_t ntable, int32_t Dp, int32_t metric, const int32_t *cand, const float *dist, int64_t n, int32_t K,
                  int32_t m, float alpha, uint8_t *keep);
int lm_link_ref(const float *table, int32_t Dp, int32_t metric, int32_t *adj, float *dist, int32_t *deg, int64_t n, int32_t cap,
                const int32_t *src, const int32_t *dst, const float *w, int64_t ne, float alpha);

static int in_range(int64_t v, int64_t n) { return v >= 0 && v < n; }

/* step 1 */
void lm_insert_ref_queries(const float *table, int32_t Dp, int32_t d, int64_t n, const int32_t *batch, int64_t b, float *q) {
    for (int64_t i = 0; i < b; ++i)
        for (int32_t c = 0; c < d; ++c) q[i * d + c] = in_range(batch[i], n) ? table[(size_t)batch[i] * (size_t)Dp + (size_t)c] : 0.0f;
}

typedef struct {
    int32_t id; /* -1: empty */
    float d;
} entry_t;

/* metric: 0 = inner product, 1 = L2 (LM_METRIC_*).  cand / cdist / keep [b][K] are outputs (never NULL here). */
int lm_insert_ref(const float *table, int32_t Dp, int32_t metric, int64_t n, int32_t cap, const int32_t *batch, int64_t b, int32_t replace, int32_t kk,
                  int32_t m, float alpha, const int64_t *s_labels, const float *s_dist, int32_t *adj, float *dist, int32_t *deg, int32_t *cand,
                  float *cdist, uint8_t *keep) {
    if (n < 1 || cap < 1 || b < 0 || kk < 1 || m < 1 || (replace != 0 && replace != 1)) return -1;
    if (b == 0) return 0;
    const int32_t K = kk + (replace ? cap : 0);
    entry_t *e = (entry_t *)malloc(sizeof(entry_t) * (size_t)K);
    entry_t *o = (entry_t *)malloc(sizeof(entry_t) * (size_t)K);
    if (!e || !o) return -2;
    /* 3-5 */
    for (int64_t i = 0; i < b; ++i) {
        const int64_t v = batch[i];
        const int live = in_range(v, n);
        for (int32_t p = 0; p < K; ++p) {
            e[p].id = -1;
            e[p].d = INFINITY;
            if (!live) continue;
            if (p < kk) {
                const int64_t lab = s_labels[i * kk + p];
                if (!in_range(lab, n) || (replace && lab == v)) continue;
                e[p].id = (int32_t)lab;
                e[p].d = metric == 1 ? s_dist[i * kk + p] : -s_dist[i * kk + p];
            } else {
                const int32_t u = adj[v * cap + (p - kk)];
                if (!in_range(u, n)) continue;
                e[p].id = u;
                e[p].d = dist[v * cap + (p - kk)];
            }
        }
        int32_t no = 0;
        if (replace) {
            for (int32_t p = K - 1; p >= 0; --p) { /* a later occurrence goes; judged on the ids as they came, so from the back */
                if (e[p].id < 0) continue;
                for (int32_t x = 0; x < p; ++x)
                    if (e[x].id == e[p].id) {
                        e[p].id = -1;
                        break;
                    }
            }
            for (int32_t p = 0; p < K; ++p) { /* stable insertion by distance: an equal distance stays behind the earlier position */
                if (e[p].id < 0 || !isfinite(e[p].d)) continue;
                int32_t at = no;
                while (at > 0 && e[p].d < o[at - 1].d) { /* (-0 < +0 is false: they count as equal) */
                    o[at] = o[at - 1];
                    --at;
                }
                o[at] = e[p];
                ++no;
            }
            for (int32_t p = no; p < K; ++p) {
                o[p].id = -1;
                o[p].d = INFINITY;
            }
        } else {
            for (int32_t p = 0; p < K; ++p) {
                o[p] = e[p];
                if (o[p].id < 0 || !isfinite(o[p].d)) {
                    o[p].id = -1;
                    o[p].d = INFINITY;
                }
            }
        }
        for (int32_t p = 0; p < K; ++p) {
            cand[i * K + p] = o[p].id;
            cdist[i * K + p] = o[p].d;
        }
    }
    free(e);
    free(o);
    /* 6 */
    int rc = lm_select_ref(table, n, Dp, metric, cand, cdist, b, K, m, alpha, keep);
    if (rc) return rc;
    /* 7 */
    const int64_t ne = 2 * b * m;
    int32_t *src = (int32_t *)malloc(sizeof(int32_t) * (size_t)ne);
    int32_t *dst = (int32_t *)malloc(sizeof(int32_t) * (size_t)ne);
    float *w = (float *)malloc(sizeof(float) * (size_t)ne);
    if (!src || !dst || !w) return -2;
    for (int64_t t = 0; t < ne; ++t) {
        src[t] = dst[t] = -1;
        w[t] = 0.0f;
    }
    for (int64_t i = 0; i < b; ++i) {
        if (!in_range(batch[i], n)) continue;
        int32_t r = 0;
        for (int32_t p = 0; p < K && r < m; ++p) {
            if (!keep[i * K + p]) continue;
            src[i * m + r] = batch[i];
            dst[i * m + r] = cand[i * K + p];
            src[b * m + i * m + r] = cand[i * K + p];
            dst[b * m + i * m + r] = batch[i];
            w[i * m + r] = w[b * m + i * m + r] = cdist[i * K + p];
            ++r;
        }
    }
    /* 8 */
    if (replace)
        for (int64_t i = 0; i < b; ++i) {
            const int64_t v = batch[i];
            if (!in_range(v, n)) continue;
            for (int32_t c = 0; c < cap; ++c) {
                adj[v * cap + c] = -1;
                dist[v * cap + c] = INFINITY;
            }
            deg[v] = 0;
        }
    /* 9 */
    rc = lm_link_ref(table, Dp, metric, adj, dist, deg, n, cap, src, dst, w, ne, alpha);
    free(src);
    free(dst);
    free(w);
    return rc;
}
