// A stand-alone caller of every host-pointer entry point ON ONE INDEX for the HOST build of the library (tests/hip_emul/build_emul_lib.py),
// meant to be built and run under AddressSanitizer with leak detection: the entry points share the index's grow-only device buffers (query /
// result staging, the padded queries, the uploaded allow-list, the per-query counters, the workspaces), so a buffer that is too small for the
// call that reuses it is a heap overflow (the emulated hipMalloc allocates the exact size), a stale capacity is a use after free, and a buffer
// that lm_index_free forgets is a leak.
//     python tests/hip_emul/build_emul_lib.py <dir> --sanitize address
//     clang++ -std=c++17 -O1 -g -pthread -fsanitize=address -shared-libsan -Iinclude tests/hip_emul/run_buffer_reuse.cpp
//         <dir>/libleann_mi355x_emul_address.so -Wl,-rpath,<dir> -o run_buffer_reuse && ./run_buffer_reuse
// N = 400, D = 48 (padded to 64: the padding buffer is in use), the two-level ring-with-chords graph of run_filtered_search.cpp, a stored f32
// table, PQ with m = 4, a host provider.  For k = 3, then 10, and n = 1, 5, 2, 9 (grow, reuse while larger than needed, grow again) every entry
// point is called in turn -- each call's shared buffers were last written by another entry point -- with the allow-list going round NULL, all
// ones, every third node.  Every call's labels and distance bits must equal the same call on a fresh index made for that call alone.  Then a
// hub cache, and a view index (lm_index_create_view) over the same graph as level arrays, under the same checks.  Test infrastructure only.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "leann_mi355x.h"

static const int N = 400, D = 48, DP = 64, M = 4, DEG0 = 7, DEG1 = 3;
static std::vector<float> g_table, g_codebooks, g_rows;
static std::vector<uint8_t> g_codes;
static std::vector<int32_t> g_levels, g_neighbors;
static std::vector<uint64_t> g_node_offsets, g_level_ptr;

// rows of the provider are d_padded wide
static int provider(void*, const int32_t* ids, int32_t n, void** out, void*) {
    g_rows.assign((size_t)n * DP, 0.0f);
    for (int i = 0; i < n; ++i) std::memcpy(&g_rows[(size_t)i * DP], &g_table[(size_t)ids[i] * D], D * sizeof(float));
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

static lm_index* make_index() {
    lm_index* idx = nullptr;
    const int rc = lm_index_create_from_csr(N, D, LM_METRIC_L2, g_node_offsets.data(), g_level_ptr.data(), (int64_t)g_level_ptr.size(), g_neighbors.data(),
                                            (int64_t)g_neighbors.size(), g_levels.data(), 0, 1, 0, &idx);
    if (rc != LM_OK) {
        std::printf("FAIL: create rc=%d %s\n", rc, lm_last_error());
        std::exit(1);
    }
    CHECK(lm_index_attach_table(idx, g_table.data(), LM_DTYPE_F32, N, D, 0) == LM_OK, "attach_table: %s", lm_last_error());
    CHECK(lm_index_set_provider(idx, provider, nullptr) == LM_OK, "set_provider");
    CHECK(lm_index_set_option(idx, "pq_threads", 256) == LM_OK, "pq_threads");
    CHECK(lm_pq_attach(idx, M, g_codebooks.data(), g_codes.data(), N) == LM_OK, "pq_attach: %s", lm_last_error());
    return idx;
}

enum Op { SEARCH_STORED, SEARCH_RECOMPUTE, SEARCH_STORED_PRUNE, SEARCH_RECOMPUTE_PRUNE, SEARCH_PROFILED, FILTERED, EXACT, PQ, PQ_FILTERED, PQ_FLAT, N_OPS };
static const char* const OP_NAME[N_OPS] = {"search stored", "search recompute", "search stored pruned", "search recompute pruned", "search profiled",
                                           "search_filtered", "search_exact", "pq_batch_search", "pq_batch_search_filtered", "pq_flat_search"};

// one call; the outputs are n x k
static int call(lm_index* idx, int op, int n, const float* q, int k, const uint32_t* allow, float* dist, int64_t* lab) {
    lm_search_params p;
    lm_search_params_default(&p);
    p.efSearch = 16;
    lm_pq_search_params pp;
    lm_pq_search_params_default(&pp);
    pp.complexity = 24;
    switch (op) {
        case SEARCH_STORED: p.recompute = 0; return lm_index_search(idx, n, q, k, dist, lab, &p);
        case SEARCH_RECOMPUTE: return lm_index_search(idx, n, q, k, dist, lab, &p);
        case SEARCH_STORED_PRUNE: p.recompute = 0; p.pq_pruning_ratio = 0.5f; return lm_index_search(idx, n, q, k, dist, lab, &p);
        case SEARCH_RECOMPUTE_PRUNE: p.pq_pruning_ratio = 0.5f; return lm_index_search(idx, n, q, k, dist, lab, &p);
        case SEARCH_PROFILED: {  // the lock-step rounds: the ones that stamp every update launch
            lm_index_set_profiling(idx, 1);
            const int rc = lm_index_search(idx, n, q, k, dist, lab, &p);
            lm_index_set_profiling(idx, 0);
            return rc;
        }
        case FILTERED: p.recompute = n % 2; return lm_index_search_filtered(idx, n, q, k, allow, dist, lab, &p);
        case EXACT: return lm_index_search_exact(idx, n, q, k, allow, dist, lab);
        case PQ: return lm_pq_batch_search(idx, n, q, k, &pp, lab, dist);
        case PQ_FILTERED: return lm_pq_batch_search_filtered(idx, n, q, k, &pp, allow, lab, dist);
        default: return lm_pq_flat_search(idx, n, q, k, &pp, allow, lab, dist);
    }
}

int main() {
    g_table.resize((size_t)N * D);
    uint32_t s = 12345;
    auto rnd = [&] { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / 16777216.0f - 0.5f; };
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < D; ++j) g_table[(size_t)i * D + j] = std::cos(6.2831853f * i / N + 0.37f * j) + 0.3f * rnd();
    // the graph twice: compact CSR, and fixed-capacity level arrays for the view
    g_levels.resize(N);
    g_node_offsets.assign(N + 1, 0);
    std::vector<int32_t> adj0, nodes1, adj1;
    for (int i = 0; i < N; ++i) {
        g_levels[i] = i % 16 == 0 ? 2 : 1;
        g_node_offsets[i + 1] = g_node_offsets[i] + g_levels[i] + 1;
        g_level_ptr.push_back(g_neighbors.size());
        for (int dlt : {1, N - 1, 2, N - 2, 7, 31, N - 45}) {
            g_neighbors.push_back((i + dlt) % N);
            adj0.push_back((i + dlt) % N);
        }
        if (g_levels[i] == 2) {
            g_level_ptr.push_back(g_neighbors.size());
            nodes1.push_back(i);
            for (int dlt : {16, N - 16, 64}) {
                g_neighbors.push_back((i + dlt) % N);
                adj1.push_back((i + dlt) % N);
            }
        }
        g_level_ptr.push_back(g_neighbors.size());
    }
    // PQ: a codebook entry of chunk j is a table row's chunk, a node's code the entry nearest to it among a few -- crude, and all the ADC needs
    g_codebooks.resize((size_t)256 * D);
    g_codes.resize((size_t)N * M);
    const int dsub = D / M;
    for (int j = 0; j < M; ++j)
        for (int c = 0; c < 256; ++c)
            for (int t = 0; t < dsub; ++t) g_codebooks[((size_t)j * 256 + c) * dsub + t] = g_table[(size_t)((c * 25 + j) % N) * D + j * dsub + t];
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < M; ++j) {
            int best = 0;
            float bd = INFINITY;
            for (int c = 0; c < 256; ++c) {
                float dd = 0;
                for (int t = 0; t < dsub; ++t) {
                    const float df = g_codebooks[((size_t)j * 256 + c) * dsub + t] - g_table[(size_t)i * D + j * dsub + t];
                    dd += df * df;
                }
                if (dd < bd) { bd = dd; best = c; }
            }
            g_codes[(size_t)i * M + j] = (uint8_t)best;
        }
    const int NMAX = 9;
    std::vector<float> q((size_t)NMAX * D);
    for (int i = 0; i < NMAX; ++i)
        for (int j = 0; j < D; ++j) q[(size_t)i * D + j] = g_table[(size_t)((37 + 71 * i) % N) * D + j] + 0.05f * rnd();
    std::vector<uint32_t> ones((N + 31) / 32, 0xFFFFFFFFu), third((N + 31) / 32, 0u);
    for (int i = 0; i < N; ++i)
        if (i % 3 == 0) third[i >> 5] |= 1u << (i & 31);
    const uint32_t* const allows[3] = {nullptr, ones.data(), third.data()};

    // ---- phase 1: every host-pointer entry point on one CSR index ----
    lm_index* shared = make_index();
    int turn = 0, ncalls = 0;
    auto both = [&](int op, int n, int k, const uint32_t* allow, lm_index* fresh_or_null, const char* what) {
        std::vector<float> ds((size_t)n * k, -1.0f), df((size_t)n * k, -2.0f);
        std::vector<int64_t> ls((size_t)n * k, -7), lf((size_t)n * k, -8);
        const int rs = call(shared, op, n, q.data(), k, allow, ds.data(), ls.data());
        CHECK(rs == LM_OK, "%s n=%d k=%d on the shared index: rc=%d %s", what, n, k, rs, lm_last_error());
        lm_index* fresh = fresh_or_null ? fresh_or_null : make_index();
        const int rf = call(fresh, op, n, q.data(), k, allow, df.data(), lf.data());
        CHECK(rf == LM_OK, "%s n=%d k=%d on a fresh index: rc=%d %s", what, n, k, rf, lm_last_error());
        if (!fresh_or_null) lm_index_free(fresh);
        CHECK(ls == lf, "%s n=%d k=%d: labels differ from a fresh index's", what, n, k);
        CHECK(!std::memcmp(ds.data(), df.data(), ds.size() * 4), "%s n=%d k=%d: distance bits differ from a fresh index's", what, n, k);
        int found = 0;
        for (int64_t v : ls) found += v >= 0;
        CHECK(found > 0, "%s n=%d k=%d: no hit at all", what, n, k);
        ++ncalls;
    };
    for (int k : {3, 10})
        for (int n : {1, 5, 2, 9}) {
            for (int i = 0; i < N_OPS; ++i) {
                // lm_index_search's five forms (ops 0 .. 4) alternate with the five other entry points (5 .. 9); where each list starts moves with every turn
                const int op = (i % 2) * 5 + (i / 2 + turn) % 5;
                both(op, n, k, allows[(turn + i) % 3], nullptr, OP_NAME[op]);
            }
            ++turn;
        }
    // the hub-embedding cache (rows d_padded wide) and the memo slots it initialises
    {
        std::vector<int32_t> hubs;
        for (int i = 0; i < N; i += 16) hubs.push_back(i);
        std::vector<float> emb(hubs.size() * DP, 0.0f);
        for (size_t h = 0; h < hubs.size(); ++h) std::memcpy(&emb[h * DP], &g_table[(size_t)hubs[h] * D], D * sizeof(float));
        lm_index* fresh = make_index();
        CHECK(lm_index_set_hub_cache(shared, hubs.data(), (int32_t)hubs.size(), emb.data()) == LM_OK, "hub cache: %s", lm_last_error());
        CHECK(lm_index_set_hub_cache(fresh, hubs.data(), (int32_t)hubs.size(), emb.data()) == LM_OK, "hub cache: %s", lm_last_error());
        both(SEARCH_RECOMPUTE, 5, 10, nullptr, fresh, "search recompute with a hub cache");
        lm_index_free(fresh);
    }
    lm_index_free(shared);

    // ---- phase 2: a view over the same graph ----
    const lm_graph_level levels[2] = {{nullptr, adj0.data(), N, DEG0}, {nodes1.data(), adj1.data(), (int64_t)nodes1.size(), DEG1}};
    auto make_view = [&] {
        lm_index* v = nullptr;
        const int rc = lm_index_create_view(N, D, LM_METRIC_L2, levels, 2, 0, 0, &v);
        if (rc != LM_OK) {
            std::printf("FAIL: create_view rc=%d %s\n", rc, lm_last_error());
            std::exit(1);
        }
        CHECK(lm_index_attach_table(v, g_table.data(), LM_DTYPE_F32, N, D, 0) == LM_OK, "attach_table (view): %s", lm_last_error());
        return v;
    };
    lm_index* view = make_view();
    lm_index* csr = make_index();
    for (int k : {3, 10})
        for (int n : {1, 5, 2, 9}) {
            std::vector<float> ds((size_t)n * k, -1.0f), df((size_t)n * k, -2.0f), dc((size_t)n * k, -3.0f);
            std::vector<int64_t> ls((size_t)n * k, -7), lf((size_t)n * k, -8), lc((size_t)n * k, -9);
            lm_index* fresh = make_view();
            CHECK(call(view, SEARCH_STORED, n, q.data(), k, nullptr, ds.data(), ls.data()) == LM_OK, "view n=%d k=%d: %s", n, k, lm_last_error());
            CHECK(call(fresh, SEARCH_STORED, n, q.data(), k, nullptr, df.data(), lf.data()) == LM_OK, "fresh view n=%d k=%d: %s", n, k, lm_last_error());
            CHECK(call(csr, SEARCH_STORED, n, q.data(), k, nullptr, dc.data(), lc.data()) == LM_OK, "CSR n=%d k=%d: %s", n, k, lm_last_error());
            lm_index_free(fresh);
            CHECK(ls == lf && !std::memcmp(ds.data(), df.data(), ds.size() * 4), "view n=%d k=%d: differs from a fresh view's", n, k);
            CHECK(ls == lc && !std::memcmp(ds.data(), dc.data(), ds.size() * 4), "view n=%d k=%d: differs from the CSR index of the same graph", n, k);
            ++ncalls;
        }
    lm_index_free(csr);
    lm_index_free(view);
    std::printf("%d calls compared\n", ncalls);
    std::printf(failures ? "FAILED\n" : "ALL OK\n");
    return failures ? 1 : 0;
}
