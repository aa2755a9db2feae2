// A stand-alone caller of lm_graph_prune_hubs for the HOST build of the library (tests/hip_emul/build_emul_lib.py: every GPU lane an OS
// thread, the kernels' own barriers the only synchronisation), meant to be built and run under ThreadSanitizer: a missing or misplaced
// barrier in the LDS histogram of the radix select, in the scan's tile hand-over or in the LDS steps of the hub sort is a data race.
//     python tests/hip_emul/build_emul_lib.py <dir> --sanitize thread
//     clang++ -std=c++17 -O1 -g -pthread -fsanitize=thread -Iinclude tests/hip_emul/run_prune.cpp <dir>/libleann_mi355x_emul_thread.so
//         -Wl,-rpath,<dir> -o run_prune && ./run_prune
// The graph: N = 1100 points on a line (point i sits at coordinate i of dimension 0), squared L2, cap 4.  Row i holds: slot 0 a hole (-1),
// slot 1 its successor i + 1 (N in the last row: out of range, empty), slot 2 itself (a self link: not usable), slot 3 node 0 for i >= 2.
// In-degrees: node 0 has N - 2 (a star), every other node 1.  With n_hubs = 600 the hubs are node 0 and then, the tie going to the lower
// id, nodes 1 .. 599 -- more than two scan tiles of nodes, more than one sort tile of keys.  Hubs keep both usable links, the others
// (m_low = 1) their first.  The answer is known by hand (distances (i - j)^2, exact in fp32 and from an fp16 table):
//   row 0: 600 candidates, the 8 nearest are 1 .. 8, and 1 dominates the rest                -> [1]
//   row 1: successor 2 and the reverse of 0 -> 1, both at distance 1, the lower id first      -> [0, 2]
//   rows 2 .. 599: predecessor, successor, node 0                                             -> [i - 1, i + 1, 0]
//   rows 600 .. N - 2: predecessor, successor                                                 -> [i - 1, i + 1]
//   row N - 1: its first usable link is node 0; the reverse of (N - 2) -> (N - 1)            -> [N - 2, 0]
// Test infrastructure only.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "leann_mi355x.h"

static const int N = 1100, D = 64, CAP = 4, M_LOW = 1, N_HUBS = 600;

static int failures = 0;
#define CHECK(cond, ...)                       \
    do {                                       \
        if (!(cond)) {                         \
            if (failures < 20) {               \
                std::printf("FAIL: " __VA_ARGS__); \
                std::printf("\n");             \
            }                                  \
            ++failures;                        \
        }                                      \
    } while (0)

// IEEE half of a small non-negative integer (exact up to 2048)
static uint16_t half_of_int(int v) {
    if (v == 0) return 0;
    int e = 0;
    while ((v >> (e + 1)) != 0) ++e;
    const uint32_t mant = ((uint32_t)v << (10 - e)) & 0x3FFu;
    return (uint16_t)(((uint32_t)(e + 15) << 10) | mant);
}

static void expected_row(int i, int32_t (&ids)[CAP], float (&d)[CAP], int& deg) {
    for (int c = 0; c < CAP; ++c) {
        ids[c] = -1;
        d[c] = INFINITY;
    }
    auto put = [&](int c, int id) {
        ids[c] = id;
        d[c] = (float)(i - id) * (float)(i - id);
    };
    if (i == 0) {
        put(0, 1);
        deg = 1;
    } else if (i == 1) {
        put(0, 0);
        put(1, 2);
        deg = 2;
    } else if (i < N_HUBS) {
        put(0, i - 1);
        put(1, i + 1);
        put(2, 0);
        deg = 3;
    } else if (i < N - 1) {
        put(0, i - 1);
        put(1, i + 1);
        deg = 2;
    } else {
        put(0, N - 2);
        put(1, 0);
        deg = 2;
    }
}

int main() {
    std::vector<float> table((size_t)N * D, 0.0f);
    std::vector<uint16_t> table16((size_t)N * D, 0);
    for (int i = 0; i < N; ++i) {
        table[(size_t)i * D] = (float)i;
        table16[(size_t)i * D] = half_of_int(i);
    }
    std::vector<int32_t> adj((size_t)N * CAP, -1);
    for (int i = 0; i < N; ++i) {
        adj[(size_t)i * CAP + 1] = i + 1;
        adj[(size_t)i * CAP + 2] = i;
        if (i >= 2) adj[(size_t)i * CAP + 3] = 0;
    }
    const size_t need = lm_graph_prune_hubs_workspace_bytes(N, CAP, M_LOW, N_HUBS);
    CHECK(need > 0, "workspace size");
    std::vector<uint64_t> ws(need / 8 + 1);
    for (int variant = 0; variant < 3; ++variant) {  // fp32 table; fp16 table; fp32 without the optional outputs
        const bool f16 = variant == 1, optional = variant != 2;
        std::vector<int32_t> a((size_t)N * CAP, 77), deg(N, 77), hubs(N_HUBS, 77), indeg(N, 77);
        std::vector<float> d((size_t)N * CAP, 7.5f);
        std::memset(ws.data(), 0xEE, ws.size() * 8);
        const int rc = lm_graph_prune_hubs(f16 ? (const void*)table16.data() : (const void*)table.data(), f16 ? LM_DTYPE_F16 : LM_DTYPE_F32, D, LM_METRIC_L2, adj.data(), N,
                                           CAP, M_LOW, N_HUBS, 1.0f, a.data(), d.data(), deg.data(), optional ? hubs.data() : nullptr, optional ? indeg.data() : nullptr,
                                           ws.data(), need, nullptr);
        if (rc != LM_OK) {
            std::printf("FAIL: variant %d rc=%d %s\n", variant, rc, lm_last_error());
            return 1;
        }
        for (int i = 0; i < N; ++i) {
            int32_t ids[CAP];
            float dd[CAP];
            int dg;
            expected_row(i, ids, dd, dg);
            CHECK(deg[i] == dg, "variant %d row %d: deg %d, expected %d", variant, i, deg[i], dg);
            for (int c = 0; c < CAP; ++c) {
                CHECK(a[(size_t)i * CAP + c] == ids[c], "variant %d row %d slot %d: id %d, expected %d", variant, i, c, a[(size_t)i * CAP + c], ids[c]);
                CHECK(!std::memcmp(&d[(size_t)i * CAP + c], &dd[c], 4), "variant %d row %d slot %d: distance %.9g, expected %.9g", variant, i, c, d[(size_t)i * CAP + c], dd[c]);
            }
            if (optional) CHECK(indeg[i] == (i == 0 ? N - 2 : 1), "variant %d: indeg[%d] = %d", variant, i, indeg[i]);
        }
        for (int i = 0; i < N_HUBS; ++i) CHECK(hubs[i] == (optional ? i : 77), "variant %d: hubs[%d] = %d", variant, i, hubs[i]);
        if (!optional) CHECK(indeg[0] == 77 && indeg[N - 1] == 77, "variant %d: d_indeg written though NULL was passed", variant);
        std::printf("variant %d (f16=%d, optional outputs=%d): %d failures so far\n", variant, (int)f16, (int)optional, failures);
    }
    std::printf(failures ? "FAILED\n" : "ALL OK\n");
    return failures ? 1 : 0;
}
