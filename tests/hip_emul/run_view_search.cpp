// A stand-alone caller of the view index (lm_index_create_view) for the HOST build of the library (tests/hip_emul/build_emul_lib.py: every
// GPU lane an OS thread, the kernels' own barriers the only synchronisation), meant to be built and run under ThreadSanitizer: a missing or
// misplaced barrier in the dense-level accessor of k_search_table -- the compaction of an upper-level row into the new-list, the popped
// ids that every wave of the level-0 hop reads -- is a data race.
//     python tests/hip_emul/build_emul_lib.py <dir> --sanitize thread
//     clang++ -std=c++17 -O1 -g -pthread -fsanitize=thread -Iinclude tests/hip_emul/run_view_search.cpp <dir>/libleann_mi355x_emul_thread.so
//         -Wl,-rpath,<dir> -o run_view_search && ./run_view_search
// The graph: 200 points on a line (point i sits at coordinate i of dimension 0), squared L2.  Level 0: row i links i - 1 and i + 1, in slots
// 1 and 3 of 6 (the others empty: -1, or a value past ntotal); level 1 lists every 8th node, its rows 70 slots wide -- wider than a wave, so
// the wave form compacts a row in two steps -- with v - 8 in slot 2 and v + 8 in slot 67; level 2 lists node 0 alone, with an empty row.
// The k = 5 nearest points of a query on the line are known by hand (ties go to the lower id): that is the embedded answer; distances are
// (q - i)^2 in fp32, what the canonical reduction gives for a vector with one non-zero coordinate.  Both workgroup forms, beam 1 and 4,
// max_batch 0 and 2, an fp32 and an fp16 table.  Test infrastructure only.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "leann_mi355x.h"

static const int N = 200, D = 64, CAP0 = 6, CAP1 = 70, K = 5, NQ = 5;

static int failures = 0;
#define CHECK(cond, ...)                  \
    do {                                  \
        if (!(cond)) {                    \
            std::printf("FAIL: " __VA_ARGS__); \
            std::printf("\n");            \
            ++failures;                   \
        }                                 \
    } while (0)

// IEEE half of a small non-negative integer (exact up to 2048)
static uint16_t half_of_int(int v) {
    if (v == 0) return 0;
    int e = 0;
    while ((v >> (e + 1)) != 0) ++e;
    const uint32_t mant = ((uint32_t)v << (10 - e)) & 0x3FFu;
    return (uint16_t)(((uint32_t)(e + 15) << 10) | mant);
}

int main() {
    std::vector<float> table((size_t)N * D, 0.0f);
    std::vector<uint16_t> table16((size_t)N * D, 0);
    for (int i = 0; i < N; ++i) {
        table[(size_t)i * D] = (float)i;
        table16[(size_t)i * D] = half_of_int(i);
    }
    std::vector<int32_t> adj0((size_t)N * CAP0, -1);
    for (int i = 0; i < N; ++i) {
        adj0[(size_t)i * CAP0 + 1] = i - 1;  // -1 at i = 0: an empty slot
        adj0[(size_t)i * CAP0 + 3] = i + 1;  // N at the last node: out of range, an empty slot
        adj0[(size_t)i * CAP0 + 4] = N + 5;
    }
    std::vector<int32_t> nodes1, adj1;
    for (int v = 0; v < N; v += 8) nodes1.push_back(v);
    adj1.assign(nodes1.size() * CAP1, -1);
    for (size_t r = 0; r < nodes1.size(); ++r) {
        adj1[r * CAP1 + 2] = nodes1[r] - 8;  // -8 at node 0: empty
        adj1[r * CAP1 + 67] = nodes1[r] + 8 < N ? nodes1[r] + 8 : -1;
    }
    const int32_t nodes2[1] = {0};
    const int32_t adj2[3] = {-1, -1, -1};
    const lm_graph_level levels[3] = {{nullptr, adj0.data(), N, CAP0}, {nodes1.data(), adj1.data(), (int64_t)nodes1.size(), CAP1}, {nodes2, adj2, 1, 3}};

    const float qpos[NQ] = {37.2f, 150.7f, 0.1f, 199.4f, 100.5f};
    const int64_t expect[NQ][K] = {{37, 38, 36, 39, 35}, {151, 150, 152, 149, 153}, {0, 1, 2, 3, 4}, {199, 198, 197, 196, 195}, {100, 101, 99, 102, 98}};
    std::vector<float> q((size_t)NQ * D, 0.0f);
    for (int i = 0; i < NQ; ++i) q[(size_t)i * D] = qpos[i];

    for (int f16 = 0; f16 < 2; ++f16) {
        lm_index* idx = nullptr;
        int rc = lm_index_create_view(N, D, LM_METRIC_L2, levels, 3, 0, 0, &idx);
        if (rc != LM_OK) {
            std::printf("FAIL: create rc=%d %s\n", rc, lm_last_error());
            return 1;
        }
        lm_index_info_t info;
        CHECK(lm_index_info(idx, &info) == LM_OK && info.max_level == 2 && info.max_degree0 == CAP0 && info.max_degree_up == CAP1 &&
                  info.n_neighbors == (int64_t)N * CAP0 + (int64_t)nodes1.size() * CAP1 + 3,
              "lm_index_info");
        CHECK(lm_index_attach_table(idx, f16 ? (const void*)table16.data() : (const void*)table.data(), f16 ? LM_DTYPE_F16 : LM_DTYPE_F32, N, D, 0) == LM_OK,
              "attach_table: %s", lm_last_error());
        struct Cfg { int wave, beam, ef, max_batch; };
        const Cfg cfgs[] = {{0, 1, 8, 0}, {0, 4, 12, 2}, {1, 1, 8, 2}, {1, 4, 12, 0}};
        for (const Cfg& c : cfgs) {
            CHECK(lm_index_set_option(idx, "persistent_wave", c.wave) == LM_OK, "set_option");
            lm_search_params p;
            lm_search_params_default(&p);
            p.efSearch = c.ef; p.beam_size = c.beam; p.recompute = 0; p.max_batch = c.max_batch;
            std::vector<float> dist((size_t)NQ * K);
            std::vector<int64_t> lab((size_t)NQ * K);
            CHECK(lm_index_search(idx, NQ, q.data(), K, dist.data(), lab.data(), &p) == LM_OK, "search: %s", lm_last_error());
            for (int i = 0; i < NQ; ++i)
                for (int j = 0; j < K; ++j) {
                    const float diff = (float)expect[i][j] - qpos[i];
                    const float want = diff * diff;
                    CHECK(lab[(size_t)i * K + j] == expect[i][j], "f16=%d wave=%d beam=%d: query %d place %d: label %lld, expected %lld", f16, c.wave, c.beam, i, j,
                          (long long)lab[(size_t)i * K + j], (long long)expect[i][j]);
                    CHECK(!std::memcmp(&dist[(size_t)i * K + j], &want, 4), "f16=%d wave=%d beam=%d: query %d place %d: distance %.9g, expected %.9g", f16, c.wave,
                          c.beam, i, j, dist[(size_t)i * K + j], want);
                }
            lm_search_stats st;
            CHECK(lm_index_get_stats(idx, &st) == LM_OK && st.ndis > NQ && st.nexpand > 0, "stats");
            std::printf("f16=%d wave=%d beam=%d ef=%d max_batch=%d: ndis %lld, nexpand %lld, nrounds %lld\n", f16, c.wave, c.beam, c.ef, c.max_batch, (long long)st.ndis,
                        (long long)st.nexpand, (long long)st.nrounds);
        }
        // a search the view does not serve leaves the outputs alone
        lm_search_params p;
        lm_search_params_default(&p);  // recompute = 1
        float d1 = 7.5f;
        int64_t l1 = 77;
        CHECK(lm_index_search(idx, 1, q.data(), 1, &d1, &l1, &p) == LM_ESTATE && d1 == 7.5f && l1 == 77, "recompute = 1 on a view");
        lm_index_free(idx);
    }
    std::printf(failures ? "FAILED\n" : "ALL OK\n");
    return failures ? 1 : 0;
}
