// A stand-alone caller of the filtered PQ traversal (lm_pq_batch_search_filtered) for the HOST build of the library
// (tests/hip_emul/build_emul_lib.py: every GPU lane an OS thread, the kernels' own barriers the only synchronisation), meant to be built and
// run under ThreadSanitizer: a missing or misplaced barrier round the allowed-only list of k_pq_traverse<NTH, true> -- its staging area, the merge
// output it shares with the walk, its per-wave counts -- is a data race.
//     python tests/hip_emul/build_emul_lib.py <dir> --sanitize thread
//     clang++ -std=c++17 -O1 -g -pthread -fsanitize=thread -Iinclude tests/hip_emul/run_pq_filtered_search.cpp <dir>/libleann_mi355x_emul_thread.so
//         -Wl,-rpath,<dir> -o run_pq_filtered_search && ./run_pq_filtered_search
// A single-level graph of 900 nodes with 64 distinct random neighbours each, D = 64, m = 16, 256 lanes per query.  The collecting threshold:
// L = 8, W = 4 with a 2 %, a 10 % and a 50 % list (the walk's list is full while the allowed-only list is not; the allowed-only list full).  The
// staging overflow: W = 64 with every node and with half of them allowed, L = 1024 and L = 64 -- the second hop brings thousands of fresh nodes,
// more than the 64 staging keys per pass of 256.  Checks that need no reference: an all-ones allow-list gives lm_pq_batch_search's labels and
// distance bits; under a list every label is allowed, distances are sorted, ndis / nexpand / nrounds are the unfiltered call's, what
// post-filtering keeps heads the result, "filtered_allowed_evals" is at least the number of hits and, with every node allowed, equals ndis.
// (The bit-exact comparison with the oracle is tests/emulated_pq_filtered_cases.py's.)  Test infrastructure only.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "leann_mi355x.h"

static const int N = 900, D = 64, M = 16, DEG = 64;

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
    uint32_t s = 2024;
    auto rnd = [&] { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / 16777216.0f - 0.5f; };
    auto rndi = [&](int n) { s = s * 1664525u + 1013904223u; return (int)((s >> 8) % (uint32_t)n); };
    std::vector<float> table((size_t)N * D), codebooks((size_t)M * 256 * (D / M));
    for (auto& v : table) v = rnd();
    for (auto& v : codebooks) v = rnd();
    std::vector<uint8_t> codes((size_t)N * M);
    for (auto& c : codes) c = (uint8_t)rndi(256);
    std::vector<int32_t> levels(N, 1), neighbors;
    std::vector<uint64_t> node_offsets(N + 1, 0), level_ptr;
    for (int i = 0; i < N; ++i) {
        node_offsets[i + 1] = node_offsets[i] + 2;
        level_ptr.push_back(neighbors.size());
        std::vector<char> used(N, 0);
        used[i] = 1;
        for (int j = 0; j < DEG;) {
            const int v = rndi(N);
            if (used[v]) continue;
            used[v] = 1;
            neighbors.push_back(v);
            ++j;
        }
        level_ptr.push_back(neighbors.size());
    }
    lm_index* idx = nullptr;
    int rc = lm_index_create_from_csr(N, D, LM_METRIC_L2, node_offsets.data(), level_ptr.data(), (int64_t)level_ptr.size(), neighbors.data(),
                                      (int64_t)neighbors.size(), levels.data(), 5, 0, 0, &idx);
    if (rc != LM_OK) {
        std::printf("FAIL: create rc=%d %s\n", rc, lm_last_error());
        return 1;
    }
    CHECK(lm_index_set_option(idx, "pq_threads", 256) == LM_OK, "pq_threads");
    CHECK(lm_pq_attach(idx, M, codebooks.data(), codes.data(), N) == LM_OK, "pq_attach: %s", lm_last_error());
    CHECK(lm_index_attach_table(idx, table.data(), LM_DTYPE_F32, N, D, 0) == LM_OK, "attach_table");
    const int nq = 2;
    std::vector<float> q((size_t)nq * D);
    for (auto& v : q) v = rnd();
    const int nw = (N + 31) / 32;
    auto every = [&](int mod) {
        std::vector<uint32_t> w(nw, 0u);
        for (int i = 0; i < N; ++i)
            if (i % mod == 0) w[i >> 5] |= 1u << (i & 31);
        return w;
    };
    struct Cfg { int L, W, k, mod, skip; };  // allowed: ids divisible by mod
    const Cfg cfgs[] = {{8, 4, 8, 50, 1}, {8, 4, 8, 10, 0}, {8, 4, 5, 2, 1}, {1024, 64, 10, 1, 1}, {1024, 64, 10, 2, 0}, {64, 64, 10, 1, 0}, {64, 64, 10, 2, 1}};
    for (const Cfg& c : cfgs) {
        lm_pq_search_params p;
        lm_pq_search_params_default(&p);
        p.complexity = c.L; p.beam_width = c.W; p.skip_search_reorder = c.skip;
        const int k = c.k;
        const std::vector<uint32_t> ones = every(1), some = every(c.mod);
        std::vector<float> du((size_t)nq * k), d1(du.size()), df(du.size());
        std::vector<int64_t> lu((size_t)nq * k), l1(lu.size()), lf(lu.size());
        lm_search_stats su, s1, sf;
        int64_t evals1 = -1, evals = -1, hits = 0;
        CHECK(lm_pq_batch_search(idx, nq, q.data(), k, &p, lu.data(), du.data()) == LM_OK, "search: %s", lm_last_error());
        lm_index_get_stats(idx, &su);
        CHECK(lm_pq_batch_search_filtered(idx, nq, q.data(), k, &p, ones.data(), l1.data(), d1.data()) == LM_OK, "filtered, all ones: %s", lm_last_error());
        lm_index_get_stats(idx, &s1);
        CHECK(lm_index_get_option(idx, "filtered_allowed_evals", &evals1) == LM_OK, "get_option");
        CHECK(l1 == lu && !std::memcmp(d1.data(), du.data(), du.size() * 4), "all ones differs from lm_pq_batch_search (L=%d W=%d)", c.L, c.W);
        CHECK(evals1 == s1.ndis, "all ones: filtered_allowed_evals %lld, ndis %lld", (long long)evals1, (long long)s1.ndis);
        CHECK(lm_pq_batch_search_filtered(idx, nq, q.data(), k, &p, some.data(), lf.data(), df.data()) == LM_OK, "filtered: %s", lm_last_error());
        lm_index_get_stats(idx, &sf);
        CHECK(su.ndis == sf.ndis && su.nexpand == sf.nexpand && su.nrounds == sf.nrounds, "stats differ (L=%d W=%d)", c.L, c.W);
        CHECK(su.ndis == s1.ndis && su.nexpand == s1.nexpand && su.nrounds == s1.nrounds, "stats differ, all ones (L=%d W=%d)", c.L, c.W);
        CHECK(lm_index_get_option(idx, "filtered_allowed_evals", &evals) == LM_OK, "get_option");
        for (int i = 0; i < nq; ++i) {
            int kept = 0;
            for (int j = 0; j < k; ++j) {
                const int64_t v = lf[(size_t)i * k + j];
                if (v >= 0) {
                    ++hits;
                    CHECK(v % c.mod == 0, "label %lld is not allowed", (long long)v);
                    CHECK(j == 0 || df[(size_t)i * k + j - 1] <= df[(size_t)i * k + j], "distances not sorted");
                } else {
                    CHECK(std::isinf(df[(size_t)i * k + j]), "empty slot without +inf");
                }
                const int64_t u = lu[(size_t)i * k + j];
                if (c.skip && u >= 0 && u % c.mod == 0) {  // (PQ order: the final list's allowed entries are the best allowed of E)
                    CHECK(lf[(size_t)i * k + kept] == u, "post-filtered label %lld is not at place %d of the filtered result", (long long)u, kept);
                    ++kept;
                }
            }
        }
        CHECK(evals >= hits && hits > 0 && evals <= evals1, "filtered_allowed_evals %lld, hits %lld", (long long)evals, (long long)hits);
        std::printf("L=%d W=%d k=%d allowed 1/%d skip_search_reorder=%d: %lld hits, %lld allowed evaluations of %lld\n", c.L, c.W, k, c.mod, c.skip,
                    (long long)hits, (long long)evals, (long long)evals1);
    }
    lm_index_free(idx);
    std::printf(failures ? "FAILED\n" : "ALL OK\n");
    return failures ? 1 : 0;
}
