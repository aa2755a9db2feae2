/*
 * lm_prune_ref.c -- CPU restatement of lm_graph_prune_hubs (include/leann_mi355x.h): the LEANN paper's high-degree-preserving pruning
 * (Algorithm 3) of a level-0 adjacency.  Test infrastructure: shares no code with the kernels (leann_amd/csrc/lm_prune_impl.h).  Steps
 * 1-5 are restated here; step 6 is the unchanged tests/link_ref/lm_link_ref.c (compiled into the same object, with
 * tests/select_ref/lm_select_ref.c) called ONCE on an empty graph; the distance function is the oracle's orc_dist.
 *
 * The rules, in the words of the header:
 *   1. slot c of row v is usable when its value u is in [0, n) and u != v;
 *   2. indeg[u] = the number of usable slots whose value is u;
 *   3. H = the first n_hubs nodes under (indeg descending, id ascending);
 *   4. quota[v] = cap for v in H, else min(m_low, cap);
 *   5. row v keeps its first quota[v] usable slots; the r-th kept link (v, u) is pair j = base[v] + r: edge 2j = v -> u, edge 2j + 1 =
 *      u -> v, both with orc_dist(row u, query v) -- a NaN as the quiet NaN 0x7FC00000 --; pairs that no kept link fills are (-1, -1);
 *   6. lm_link_ref on the empty graph with all 2 * base[n] edges.
 * `table` is fp32 [n][Dp], zero padded (an fp16 table is widened by the caller: exact).
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

float orc_dist(const float *e, const float *q, int32_t Dp, int32_t metric); /* oracle/lm_oracle.c */
int lm_link_ref(const float *table, int32_t Dp, int32_t metric, int32_t *adj, float *dist, int32_t *deg, int64_t n, int32_t cap,
                const int32_t *src, const int32_t *dst, const float *w, int64_t ne, float alpha);

typedef struct {
    int32_t indeg;
    int32_t id;
} node_t;

static int by_indeg_desc_then_id(const void *pa, const void *pb) {
    const node_t *a = (const node_t *)pa, *b = (const node_t *)pb;
    if (a->indeg != b->indeg) return a->indeg > b->indeg ? -1 : 1;
    return (a->id > b->id) - (a->id < b->id);
}

static int usable(int32_t u, int64_t v, int64_t n) { return u >= 0 && u < n && u != v; }

/* hubs [n_hubs] and indeg [n] may be NULL */
int lm_prune_ref(const float *table, int32_t Dp, int32_t metric, const int32_t *adj_in, int64_t n, int32_t cap, int32_t m_low, int64_t n_hubs,
                 float alpha, int32_t *adj_out, float *dist_out, int32_t *deg_out, int32_t *hubs, int32_t *indeg_out) {
    if (n < 0 || cap < 1 || m_low < 1 || n_hubs < 0 || n_hubs > n) return -1;
    if (n == 0) return 0;
    const int32_t mq = m_low < cap ? m_low : cap;
    node_t *order = (node_t *)malloc(sizeof(node_t) * (size_t)n);
    int32_t *quota = (int32_t *)malloc(sizeof(int32_t) * (size_t)n);
    if (!order || !quota) return -2;
    /* 1 + 2 */
    for (int64_t v = 0; v < n; ++v) {
        order[v].indeg = 0;
        order[v].id = (int32_t)v;
    }
    for (int64_t v = 0; v < n; ++v)
        for (int32_t c = 0; c < cap; ++c) {
            const int32_t u = adj_in[v * cap + c];
            if (usable(u, v, n)) order[u].indeg++;
        }
    if (indeg_out)
        for (int64_t v = 0; v < n; ++v) indeg_out[v] = order[v].indeg;
    /* 3 + 4 */
    qsort(order, (size_t)n, sizeof(node_t), by_indeg_desc_then_id);
    for (int64_t v = 0; v < n; ++v) quota[v] = mq;
    for (int64_t i = 0; i < n_hubs; ++i) {
        quota[order[i].id] = cap;
        if (hubs) hubs[i] = order[i].id;
    }
    /* 5 */
    int64_t pairs = 0;
    for (int64_t v = 0; v < n; ++v) pairs += quota[v];
    const int64_t ne = 2 * pairs;
    int32_t *src = (int32_t *)malloc(sizeof(int32_t) * (size_t)ne);
    int32_t *dst = (int32_t *)malloc(sizeof(int32_t) * (size_t)ne);
    float *w = (float *)malloc(sizeof(float) * (size_t)ne);
    if (!src || !dst || !w) return -2;
    int64_t j = 0;
    for (int64_t v = 0; v < n; ++v) {
        int32_t kept = 0;
        for (int32_t c = 0; c < cap && kept < quota[v]; ++c) {
            const int32_t u = adj_in[v * cap + c];
            if (!usable(u, v, n)) continue;
            float d = orc_dist(table + (size_t)u * (size_t)Dp, table + (size_t)v * (size_t)Dp, Dp, metric);
            if (isnan(d)) { /* the header: a NaN weight is THE quiet NaN 0x7FC00000, whatever sign and payload the platform computed */
                const uint32_t qnan = 0x7FC00000u;
                memcpy(&d, &qnan, 4);
            }
            src[2 * j] = (int32_t)v;
            dst[2 * j] = u;
            src[2 * j + 1] = u;
            dst[2 * j + 1] = (int32_t)v;
            w[2 * j] = w[2 * j + 1] = d;
            ++j;
            ++kept;
        }
        for (; kept < quota[v]; ++kept, ++j) {
            src[2 * j] = dst[2 * j] = src[2 * j + 1] = dst[2 * j + 1] = -1;
            w[2 * j] = w[2 * j + 1] = 0.0f;
        }
    }
    /* 6 */
    for (int64_t t = 0; t < n * cap; ++t) {
        adj_out[t] = -1;
        dist_out[t] = INFINITY;
    }
    for (int64_t v = 0; v < n; ++v) deg_out[v] = 0;
    const int rc = lm_link_ref(table, Dp, metric, adj_out, dist_out, deg_out, n, cap, src, dst, w, ne, alpha);
    free(order);
    free(quota);
    free(src);
    free(dst);
    free(w);
    return rc;
}
