// A stand-alone caller of lm_graph_insert_batch ON ONE VIEW INDEX for the HOST build of the library (tests/hip_emul/build_emul_lib.py), meant to
// be built and run under AddressSanitizer with leak detection: the call keeps its intermediate buffers (queries, search result, candidates,
// keep mask, edges, the link insertion's workspace) with the index as grow-only buffers, so a buffer that is too small for the call that
// reuses it is a heap overflow (the emulated hipMalloc allocates the exact size), a stale capacity is a use after free, and a buffer that
// lm_index_free forgets is a leak.
//     python tests/hip_emul/build_emul_lib.py <dir> --sanitize address
//     clang++ -std=c++17 -O1 -g -pthread -fsanitize=address -shared-libsan -Iinclude tests/hip_emul/run_insert.cpp
//         <dir>/libleann_mi355x_emul_address.so -Wl,-rpath,<dir> -o run_insert && ./run_insert
// N = 400, D = 48 (padded to 64), two levels: a ring with chords in rows of cap 8 with holes, and every 20th node on a level of cap 4.  Eight
// calls on one handle, b and K growing and shrinking, replace 0 and 1, the optional outputs given or not; before every call the level
// arrays are copied, and the same call on a FRESH handle over the copy must leave the same arrays and outputs, byte for byte.
// Test infrastructure only.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "leann_mi355x.h"

static const int N = 400, D = 48, DP = 64, CAP = 8, UP = 20, UCAP = 4;
static std::vector<float> g_table;          // [N][DP], zero padded: borrowed by the handles (location 1)
static std::vector<int32_t> g_up_nodes, g_up_adj;

static int failures = 0;
#define CHECK(cond, ...)                       \
    do {                                       \
        if (!(cond)) {                         \
            std::printf("FAIL: " __VA_ARGS__); \
            std::printf("\n");                 \
            ++failures;                        \
        }                                      \
    } while (0)

struct Level0 {
    std::vector<int32_t> adj, deg;
    std::vector<float> dist;
};

static lm_index* make_view(Level0& g) {
    lm_graph_level lv[2];
    std::memset(lv, 0, sizeof(lv));
    lv[0].d_nodes = nullptr;
    lv[0].d_adj = g.adj.data();
    lv[0].n_rows = N;
    lv[0].cap = CAP;
    lv[1].d_nodes = g_up_nodes.data();
    lv[1].d_adj = g_up_adj.data();
    lv[1].n_rows = UP;
    lv[1].cap = UCAP;
    lm_index* idx = nullptr;
    const int rc = lm_index_create_view(N, D, LM_METRIC_L2, lv, 2, 0, 0, &idx);
    if (rc != LM_OK) {
        std::printf("FAIL: create_view rc=%d %s\n", rc, lm_last_error());
        std::exit(1);
    }
    CHECK(lm_index_attach_table(idx, g_table.data(), LM_DTYPE_F32, N, D, 1) == LM_OK, "attach_table: %s", lm_last_error());
    return idx;
}

struct Out {
    std::vector<int32_t> cand;
    std::vector<float> cdist;
    std::vector<uint8_t> keep;
};

static int insert(lm_index* idx, Level0& g, const std::vector<int32_t>& batch, int replace, int kk, int m, bool outputs, Out& o) {
    lm_search_params p;
    lm_search_params_default(&p);
    p.efSearch = kk > 24 ? kk : 24;
    p.beam_size = 2;
    p.recompute = 0;
    const size_t K = (size_t)kk + (replace ? CAP : 0);
    o.cand.assign(batch.size() * K, 0x6E6E6E6E);
    o.cdist.assign(batch.size() * K, 7.5f);
    o.keep.assign(batch.size() * K, 0x6E);
    return lm_graph_insert_batch(idx, batch.data(), (int64_t)batch.size(), replace, kk, m, 1.0f, &p, g.adj.data(), g.dist.data(), g.deg.data(),
                                 outputs ? o.cand.data() : nullptr, outputs ? o.cdist.data() : nullptr, outputs ? o.keep.data() : nullptr);
}

template <class T>
static bool same(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

int main() {
    g_table.assign((size_t)N * DP, 0.0f);
    uint32_t s = 12345u;
    for (int v = 0; v < N; ++v)
        for (int c = 0; c < D; ++c) {
            s = s * 1664525u + 1013904223u;
            g_table[(size_t)v * DP + c] = (float)((s >> 8) & 0xFFFF) / 65536.0f - 0.5f + 0.01f * (float)(v % 17);
        }
    Level0 g;
    g.adj.assign((size_t)N * CAP, -1);
    g.dist.assign((size_t)N * CAP, INFINITY);
    g.deg.assign(N, 0);
    for (int v = 0; v < N; ++v) {
        const int nb[4] = {(v + 1) % N, (v + N - 1) % N, (v + 7) % N, (v + 31) % N};
        const int slot[4] = {0, 2, 3, 6};  // holes at 1, 4, 5, 7
        for (int j = 0; j < 4; ++j) {
            float d2 = 0.0f;
            for (int c = 0; c < D; ++c) {
                const float t = g_table[(size_t)v * DP + c] - g_table[(size_t)nb[j] * DP + c];
                d2 += t * t;
            }
            g.adj[(size_t)v * CAP + slot[j]] = nb[j];
            g.dist[(size_t)v * CAP + slot[j]] = d2;
        }
        g.deg[v] = 4;
    }
    g.adj[5 * CAP + 1] = N + 9;  // an out-of-range slot value
    for (int r = 0; r < UP; ++r) g_up_nodes.push_back(r * (N / UP));
    g_up_adj.assign((size_t)UP * UCAP, -1);
    for (int r = 0; r < UP; ++r) {
        g_up_adj[(size_t)r * UCAP + 0] = g_up_nodes[(r + 1) % UP];
        g_up_adj[(size_t)r * UCAP + 2] = g_up_nodes[(r + UP - 1) % UP];
        g_up_adj[(size_t)r * UCAP + 3] = g_up_nodes[(r + 5) % UP];
    }

    lm_index* shared = make_view(g);
    //                     b   kk  replace  m  outputs
    const int plan[8][5] = {{5, 4, 0, 3, 1}, {24, 20, 1, 4, 1}, {3, 8, 1, 4, 0}, {33, 30, 0, 6, 1}, {1, 1, 1, 1, 1}, {48, 12, 1, 4, 1}, {7, 40, 0, 9, 0}, {16, 6, 1, 2, 1}};
    int compared = 0;
    for (int c = 0; c < 8; ++c) {
        const int b = plan[c][0], kk = plan[c][1], replace = plan[c][2], m = plan[c][3];
        const bool outputs = plan[c][4] != 0;
        std::vector<int32_t> batch;
        for (int i = 0; i < b; ++i) batch.push_back((int32_t)((i * 37 + c * 11) % N));
        if (b >= 5) {
            batch[1] = -1;        // void
            batch[2] = N + 5;     // void
            batch[4] = batch[0];  // listed twice
        }
        Level0 copy = g;
        lm_index* fresh = make_view(copy);
        Out o1, o2;
        const int rc1 = insert(shared, g, batch, replace, kk, m, outputs, o1);
        const int rc2 = insert(fresh, copy, batch, replace, kk, m, outputs, o2);
        CHECK(rc1 == LM_OK && rc2 == LM_OK, "call %d: rc %d / %d: %s", c, rc1, rc2, lm_last_error());
        CHECK(same(g.adj, copy.adj) && same(g.dist, copy.dist) && same(g.deg, copy.deg), "call %d: level arrays differ from a fresh handle's", c);
        CHECK(same(o1.cand, o2.cand) && same(o1.cdist, o2.cdist) && same(o1.keep, o2.keep), "call %d: outputs differ from a fresh handle's", c);
        if (outputs) {
            bool any = false;
            for (uint8_t k : o1.keep) {
                CHECK(k == 0 || k == 1, "call %d: keep byte %d", c, (int)k);
                any = any || k == 1;
            }
            CHECK(any, "call %d: nothing kept", c);
        } else {
            CHECK(o1.cand[0] == 0x6E6E6E6E && o1.keep[0] == 0x6E, "call %d: an output that was not given was written", c);
        }
        lm_search_stats st1, st2;
        CHECK(lm_index_get_stats(shared, &st1) == LM_OK && lm_index_get_stats(fresh, &st2) == LM_OK && st1.ndis == st2.ndis && st1.ndis > 0, "call %d: stats", c);
        lm_index_free(fresh);
        ++compared;
    }
    int total = 0;
    for (int v = 0; v < N; ++v) total += g.deg[v];
    CHECK(total > 4 * N, "the calls added no links (%d)", total);
    lm_index_free(shared);
    std::printf("%d calls compared, %d links\n", compared, total);
    if (failures) {
        std::printf("%d FAILURES\n", failures);
        return 1;
    }
    std::printf("ALL OK\n");
    return 0;
}
