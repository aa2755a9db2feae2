// A stand-alone caller of the filtered graph search (lm_index_search_filtered) for the HOST build of the library
// (tests/hip_emul/build_emul_lib.py: every GPU lane an OS thread, the kernels' own barriers the only synchronisation), meant to be built and
// run under ThreadSanitizer: a missing or misplaced barrier in k_filter_collect, or a write of it into anything the walk reads, is a data race.
//     python tests/hip_emul/build_emul_lib.py <dir> --sanitize thread
//     clang++ -std=c++17 -O1 -g -pthread -fsanitize=thread -Iinclude tests/hip_emul/run_filtered_search.cpp <dir>/libleann_mi355x_emul_thread.so
//         -Wl,-rpath,<dir> -o run_filtered_search && ./run_filtered_search
// A two-level graph of 400 nodes (ring with chords at level 0, every 16th node on level 1), D = 64, both sources (stored table, provider with
// and without the per-call memo), beam 1 and 4, dynamic batching, k above efSearch.  Checks that need no reference: an all-ones allow-list
// gives lm_index_search's labels and distance bits; under a list every label is allowed, distances are sorted, the stats are the unfiltered
// call's, what post-filtering keeps heads the result, and "filtered_allowed_evals" is at least the number of hits.  (The bit-exact comparison
// with the oracle is tests/emulated_filtered_cases.py's.)  Test infrastructure only.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "leann_mi355x.h"

static const int N = 400, D = 64;
static std::vector<float> g_table, g_rows;

static int provider(void*, const int32_t* ids, int32_t n, void** out, void*) {
    g_rows.resize((size_t)n * D);
    for (int i = 0; i < n; ++i) std::memcpy(&g_rows[(size_t)i * D], &g_table[(size_t)ids[i] * D], D * sizeof(float));
    *out = g_rows.data();
    return 0;
}

static int failures = 0;
#define CHECK(cond, ...)                  \
    do {                                  \
        if (!(cond)) {                    \
            std::printf("FAIL: " __VA_ARGS__); \
            std::printf("\n");            \
            ++failures;                   \
        }                                 \
    } while (0)

int main() {
    // vectors on a noisy circle: neighbours on the ring are near
    g_table.resize((size_t)N * D);
    uint32_t s = 12345;
    auto rnd = [&] { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / 16777216.0f - 0.5f; };
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < D; ++j) g_table[(size_t)i * D + j] = std::cos(6.2831853f * i / N + 0.37f * j) + 0.3f * rnd();
    std::vector<int32_t> levels(N), neighbors;
    std::vector<uint64_t> node_offsets(N + 1, 0), level_ptr;
    for (int i = 0; i < N; ++i) {
        levels[i] = i % 16 == 0 ? 2 : 1;
        node_offsets[i + 1] = node_offsets[i] + levels[i] + 1;
        level_ptr.push_back(neighbors.size());
        for (int dlt : {1, N - 1, 2, N - 2, 7, 31, N - 45}) neighbors.push_back((i + dlt) % N);
        if (levels[i] == 2) {
            level_ptr.push_back(neighbors.size());
            for (int dlt : {16, N - 16, 64}) neighbors.push_back((i + dlt) % N);
        }
        level_ptr.push_back(neighbors.size());
    }
    lm_index* idx = nullptr;
    int rc = lm_index_create_from_csr(N, D, LM_METRIC_L2, node_offsets.data(), level_ptr.data(), (int64_t)level_ptr.size(), neighbors.data(),
                                      (int64_t)neighbors.size(), levels.data(), 0, 1, 0, &idx);
    if (rc != LM_OK) {
        std::printf("FAIL: create rc=%d %s\n", rc, lm_last_error());
        return 1;
    }
    CHECK(lm_index_attach_table(idx, g_table.data(), LM_DTYPE_F32, N, D, 0) == LM_OK, "attach_table");
    CHECK(lm_index_set_provider(idx, provider, nullptr) == LM_OK, "set_provider");
    const int nq = 5;
    std::vector<float> q((size_t)nq * D);
    for (int i = 0; i < nq; ++i)
        for (int j = 0; j < D; ++j) q[(size_t)i * D + j] = g_table[(size_t)(37 + 71 * i) * D + j] + 0.05f * rnd();
    std::vector<uint32_t> ones((N + 31) / 32, 0xFFFFFFFFu), third((N + 31) / 32, 0u);
    for (int i = 0; i < N; ++i)
        if (i % 3 == 0) third[i >> 5] |= 1u << (i & 31);
    struct Cfg { int recompute, memo, ef, k, beam, bs, max_batch; };
    const Cfg cfgs[] = {{0, 1, 24, 5, 1, 0, 0}, {0, 1, 8, 12, 4, 16, 2}, {1, 1, 24, 5, 1, 0, 0}, {1, 0, 16, 1, 4, 16, 0}, {1, 1, 16, 5, 2, 0, 1}};
    for (const Cfg& c : cfgs) {
        lm_search_params p;
        lm_search_params_default(&p);
        p.efSearch = c.ef; p.beam_size = c.beam; p.batch_size = c.bs; p.recompute = c.recompute; p.recompute_memo = c.memo; p.max_batch = c.max_batch;
        const int k = c.k;
        std::vector<float> du((size_t)nq * k), d1(du.size()), df(du.size());
        std::vector<int64_t> lu((size_t)nq * k), l1(lu.size()), lf(lu.size());
        lm_search_stats su, sf;
        CHECK(lm_index_search(idx, nq, q.data(), k, du.data(), lu.data(), &p) == LM_OK, "search: %s", lm_last_error());
        lm_index_get_stats(idx, &su);
        CHECK(lm_index_search_filtered(idx, nq, q.data(), k, ones.data(), d1.data(), l1.data(), &p) == LM_OK, "filtered, all ones: %s", lm_last_error());
        CHECK(l1 == lu && !std::memcmp(d1.data(), du.data(), du.size() * 4), "all ones differs from lm_index_search (recompute=%d ef=%d k=%d)", c.recompute, c.ef, k);
        CHECK(lm_index_search_filtered(idx, nq, q.data(), k, third.data(), df.data(), lf.data(), &p) == LM_OK, "filtered: %s", lm_last_error());
        lm_index_get_stats(idx, &sf);
        CHECK(su.ndis == sf.ndis && su.nexpand == sf.nexpand && su.nrounds == sf.nrounds && su.nunique == sf.nunique, "stats differ (recompute=%d ef=%d k=%d)",
              c.recompute, c.ef, k);
        int64_t evals = -1, hits = 0;
        CHECK(lm_index_get_option(idx, "filtered_allowed_evals", &evals) == LM_OK, "get_option");
        for (int i = 0; i < nq; ++i) {
            int kept = 0;
            for (int j = 0; j < k; ++j) {
                const int64_t v = lf[(size_t)i * k + j];
                if (v >= 0) {
                    ++hits;
                    CHECK(v % 3 == 0, "label %lld is not allowed", (long long)v);
                    CHECK(j == 0 || df[(size_t)i * k + j - 1] <= df[(size_t)i * k + j], "distances not sorted");
                } else {
                    CHECK(std::isinf(df[(size_t)i * k + j]), "empty slot without +inf");
                }
                const int64_t u = lu[(size_t)i * k + j];
                if (u >= 0 && u % 3 == 0) {
                    CHECK(lf[(size_t)i * k + kept] == u, "post-filtered label %lld is not at place %d of the filtered result", (long long)u, kept);
                    ++kept;
                }
            }
        }
        CHECK(evals >= hits && hits > 0, "filtered_allowed_evals %lld, hits %lld", (long long)evals, (long long)hits);
        std::printf("recompute=%d memo=%d ef=%d k=%d beam=%d batch_size=%d max_batch=%d: %lld hits, %lld allowed evaluations\n", c.recompute, c.memo, c.ef, k,
                    c.beam, c.bs, c.max_batch, (long long)hits, (long long)evals);
    }
    lm_index_free(idx);
    std::printf(failures ? "FAILED\n" : "ALL OK\n");
    return failures ? 1 : 0;
}
