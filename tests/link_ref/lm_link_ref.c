/*
 * lm_link_ref.c -- CPU restatement of lm_graph_add_links (include/leann_mi355x.h): the link insertion of graph construction.
 * Test infrastructure: shares no code with the kernels (leann_amd/csrc/lm_link_impl.h).  Step 5, the shrink of an overflowing list, is
 * tests/select_ref/lm_select_ref.c (compiled into the same object), whose distance function is the oracle's orc_dist.
 *
 * The rules, in the words of the header, for every row v that is the src of at least one valid edge (src, dst in [0, n), src != dst):
 *   1. candidates: the slots of adj[v] with 0 <= id < n in slot order with dist[v][c], then the valid edges of v in ascending e with w[e];
 *   2. dedupe by dst, the first occurrence wins;
 *   3. sort by (internal distance, dst) ascending; NaN ranks as +inf, -0 as +0, ties go to the lower dst;
 *   4. truncate to 2 cap;
 *   5. at most cap left: the list as it stands; else lm_select_ref with K = 2 cap, m = cap on the candidates and their distances;
 *   6. kept entries left-packed with the distance bits they came with, the rest -1 / +inf, deg[v] = the count.
 * Rows that are not affected are not touched.  `table` is fp32 [n][Dp], zero padded (an fp16 table is widened by the caller: exact).
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

int lm_select_ref(const float *table, int64_t ntable, int32_t Dp, int32_t metric, const int32_t *cand, const float *dist, int64_t n,
                  int32_t K, int32_t m, float alpha, uint8_t *keep);

typedef struct {
    float rank; /* the distance as it is ranked: NaN -> +inf (-0 == +0 under <) */
    float w;    /* the distance as given */
    int32_t dst;
} cand_t;

static int by_rank_then_dst(const void *pa, const void *pb) {
    const cand_t *a = (const cand_t *)pa, *b = (const cand_t *)pb;
    if (a->rank < b->rank) return -1;
    if (a->rank > b->rank) return 1;
    return (a->dst > b->dst) - (a->dst < b->dst);
}

static int valid_edge(int32_t s, int32_t d, int64_t n) { return s >= 0 && s < n && d >= 0 && d < n && s != d; }

int lm_link_ref(const float *table, int32_t Dp, int32_t metric, int32_t *adj, float *dist, int32_t *deg, int64_t n, int32_t cap,
                const int32_t *src, const int32_t *dst, const float *w, int64_t ne, float alpha) {
    if (n < 0 || ne < 0 || cap < 1) return -1;
    if (n == 0 || ne == 0) return 0;
    /* edges of every row, in ascending e */
    int64_t *cnt = (int64_t *)calloc((size_t)n + 1, sizeof(int64_t));
    int64_t *pos = (int64_t *)calloc((size_t)n + 1, sizeof(int64_t));
    int64_t *by_src = (int64_t *)malloc(sizeof(int64_t) * (size_t)ne);
    if (!cnt || !pos || !by_src) return -2;
    for (int64_t e = 0; e < ne; ++e)
        if (valid_edge(src[e], dst[e], n)) cnt[src[e] + 1]++;
    for (int64_t v = 0; v < n; ++v) cnt[v + 1] += cnt[v];
    memcpy(pos, cnt, sizeof(int64_t) * ((size_t)n + 1));
    for (int64_t e = 0; e < ne; ++e)
        if (valid_edge(src[e], dst[e], n)) by_src[pos[src[e]]++] = e;
    const int K = 2 * cap;
    int rc = 0;
    /* rows are independent: row v reads and writes row v of adj / dist / deg only */
#pragma omp parallel for schedule(dynamic, 16)
    for (int64_t v = 0; v < n; ++v) {
        const int64_t m = cnt[v + 1] - cnt[v];
        if (m == 0) continue; /* not affected */
        cand_t *c = (cand_t *)malloc(sizeof(cand_t) * (size_t)(cap + m));
        int32_t *sid = (int32_t *)malloc(sizeof(int32_t) * (size_t)K);
        float *sd = (float *)malloc(sizeof(float) * (size_t)K);
        uint8_t *keep = (uint8_t *)malloc((size_t)K);
        if (!c || !sid || !sd || !keep) {
            rc = -2;
            free(c);
            free(sid);
            free(sd);
            free(keep);
            continue;
        }
        int64_t nc = 0;
        /* 1 + 2: candidates in order; one whose dst is already there loses */
        for (int64_t t = 0; t < cap + m; ++t) {
            int32_t id;
            float d;
            if (t < cap) {
                id = adj[v * cap + t];
                d = dist[v * cap + t];
                if (id < 0 || id >= n) continue;
            } else {
                const int64_t e = by_src[cnt[v] + (t - cap)];
                id = dst[e];
                d = w[e];
            }
            int seen = 0;
            for (int64_t x = 0; x < nc && !seen; ++x) seen = c[x].dst == id;
            if (seen) continue;
            c[nc].dst = id;
            c[nc].w = d;
            c[nc].rank = isnan(d) ? INFINITY : d;
            ++nc;
        }
        /* 3 + 4 (dsts are distinct now: the order is total) */
        qsort(c, (size_t)nc, sizeof(cand_t), by_rank_then_dst);
        if (nc > K) nc = K;
        /* 5 */
        for (int j = 0; j < K; ++j) {
            sid[j] = j < nc ? c[j].dst : -1;
            sd[j] = j < nc ? c[j].w : INFINITY;
            keep[j] = j < nc;
        }
        if (nc > cap && lm_select_ref(table, n, Dp, metric, sid, sd, 1, K, cap, alpha, keep) != 0) rc = -3;
        /* 6 */
        int32_t o = 0;
        for (int j = 0; j < nc; ++j)
            if (keep[j]) {
                adj[v * cap + o] = sid[j];
                dist[v * cap + o] = sd[j];
                ++o;
            }
        deg[v] = o;
        for (; o < cap; ++o) {
            adj[v * cap + o] = -1;
            dist[v * cap + o] = INFINITY;
        }
        free(c);
        free(sid);
        free(sd);
        free(keep);
    }
    free(cnt);
    free(pos);
    free(by_src);
    return rc;
}

float orc_dist(const float *e, const float *q, int32_t Dp, int32_t metric); /* oracle/lm_oracle.c */

/* out[e] = the canonical internal distance of table[src[e]] and table[dst[e]] (test inputs whose weights "come from the table") */
void lm_link_ref_pair_dists(const float *table, int32_t Dp, int32_t metric, const int32_t *src, const int32_t *dst, int64_t ne, float *out) {
    for (int64_t e = 0; e < ne; ++e) out[e] = orc_dist(table + (size_t)src[e] * (size_t)Dp, table + (size_t)dst[e] * (size_t)Dp, Dp, metric);
}
