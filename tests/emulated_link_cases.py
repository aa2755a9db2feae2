"""Link-insertion scenarios run against libleann_mi355x_emul.so (tests/hip_emul/build_emul_lib.py: the product's kernels on the CPU, a
thread per lane) and the CPU restatement tests/link_ref/lm_link_ref.c.  Imported by tests/test_link_kernel.py and runnable:
    python -m tests.emulated_link_cases <path/to/libleann_mi355x_emul.so> <path/to/liblm_link_ref.so> [case ...]
adj, dist (as bit patterns) and deg are compared byte for byte."""
import sys
from pathlib import Path

import numpy as np

CASES = {}
REF = None


def _load(lib_path: str):
    from leann_amd import _lib

    _lib.LIB_PATH = Path(lib_path)
    _lib._lib = None
    return _lib.load()


def _kernel(table, adj, dist, deg, src, dst, w, metric, alpha):
    """lm_graph_add_links through the ABI on COPIES of the numpy arrays ('device' pointers are host pointers in the emulated world)."""
    from leann_amd import _lib

    lib = _lib.load()
    table = np.ascontiguousarray(table)
    adj, dist, deg = np.array(adj, np.int32, order="C"), np.array(dist, np.float32, order="C"), np.array(deg, np.int32, order="C")
    src, dst, w = np.ascontiguousarray(src, np.int32), np.ascontiguousarray(dst, np.int32), np.ascontiguousarray(w, np.float32)
    n, cap = adj.shape
    ws = np.full(max(int(lib.lm_graph_add_links_workspace_bytes(n, src.shape[0])), 1), 0xEE, np.uint8)
    rc = lib.lm_graph_add_links(table.ctypes.data, _lib.DTYPE_F16 if table.dtype == np.float16 else _lib.DTYPE_F32, table.shape[1], metric, adj.ctypes.data,
                                dist.ctypes.data, deg.ctypes.data, n, cap, src.ctypes.data, dst.ctypes.data, w.ctypes.data, src.shape[0], alpha, ws.ctypes.data,
                                ws.shape[0], None)
    _lib.check(rc, "lm_graph_add_links")
    return adj, dist, deg


def _table(N, d, seed, f16):
    from tests.select_ref_util import pad64
    from tests.util import clustered

    x = clustered(N, d, seed, n_centers=8, sigma=0.5)
    nd = N // 6
    x[:nd] = x[nd : 2 * nd]  # duplicate vectors: exact ties
    return pad64(x.astype(np.float16) if f16 else x)


def case_kernel_vs_restatement():
    """Both metrics, fp32 / fp16 tables, alpha in {1, 1.2}, d in {48 -> 64, 384}, cap in {1, 4, 32, 64, LM_SELECT_MAX_K / 2}, on a table
    with duplicated vectors; level graph and edges from tests.link_ref_util.edge_case_inputs.  The emulation runs a thread per lane, so
    n is the smallest the edge set allows (2 cap + 40: a row with more than 2 cap distinct candidates needs that many nodes)."""
    from leann_amd import _lib
    from tests.link_ref_util import edge_case_inputs, order_preserving_permutation, ref_link, same_bytes

    combos = [(metric, f16, alpha) for metric in (0, 1) for f16 in (False, True) for alpha in (1.0, 1.2)]
    seen = set()
    run = 0
    for ci, cap in enumerate((1, 4, 32, 64, _lib.SELECT_MAX_K // 2)):
        n = max(2 * cap + 40, 120)
        for di, d in enumerate((48, 384)):
            for metric, f16, alpha in combos:  # the whole metric x dtype x alpha product at every cap and width
                table = _table(n, d, 100 + run, f16)
                inp = edge_case_inputs(REF, table, cap, metric, 300 + run, _lib.LINK_STAGE)
                args = (inp["adj"], inp["dist"], inp["deg"], inp["src"], inp["dst"], inp["w"], metric, alpha)
                got = _kernel(table, *args)
                exp = ref_link(REF, table, *args)
                ok = same_bytes(got, exp)
                u = inp["untouched"]
                ok = ok and got[0][u].tobytes() == inp["adj"][u].tobytes() and got[1][u].tobytes() == inp["dist"][u].tobytes() and got[2][u].tobytes() == inp["deg"][u].tobytes()
                # the designed rows did end where they were meant to
                for v, total in inp["designed"].items():
                    ok = ok and (got[2][v] == total if total <= cap else 1 <= got[2][v] <= cap)
                valid = (got[0] >= 0) & (got[0] < n)
                s_, d_ = inp["src"].astype(np.int64), inp["dst"].astype(np.int64)
                aff = np.unique(s_[(s_ >= 0) & (s_ < n) & (d_ >= 0) & (d_ < n) & (s_ != d_)])  # the affected rows
                ok = ok and np.array_equal(valid[aff].sum(1), got[2][aff]) and bool((got[0][aff][~valid[aff]] == -1).all())
                if run % 4 == 0:  # the same input again, and the edges in another order that keeps every duplicate pair's order: the same bytes
                    ok = ok and same_bytes(_kernel(table, *args), got)
                    o = order_preserving_permutation(inp["src"], inp["dst"], np.random.default_rng(run))
                    ok = ok and same_bytes(_kernel(table, inp["adj"], inp["dist"], inp["deg"], inp["src"][o], inp["dst"][o], inp["w"][o], metric, alpha), got)
                print(f"link cap={cap} n={n} d={d} metric={metric} f16={f16} alpha={alpha} edges={inp['src'].shape[0]} mean deg={got[2][aff].mean():.2f}: "
                      f"{'ok' if ok else 'MISMATCH'}", flush=True)
                assert ok
                seen.add((metric, f16, alpha, d, cap))
                run += 1
    assert len(seen) == 8 * 2 * 5 == run


CASES["kernel_vs_restatement"] = case_kernel_vs_restatement


def case_torch_form_agrees():
    """Weights that come from the table by the canonical reduction, no NaNs, valid edges, holes that are -1: the existing
    _LevelGraph.add_links with selector="kernel" (the torch-op composition), the restatement and the kernel produce the same rows."""
    import torch

    from leann_amd import gpu_graph_build as gb
    from tests.link_ref_util import pair_dists, ref_link, same_bytes

    run = 0
    for metric in (0, 1):
        for f16 in (False, True):
            for cap, n in ((1, 90), (4, 120), (16, 160)):
                for alpha in (1.0, 1.2):
                    rng = np.random.default_rng(50 + run)
                    table = _table(n, 48, 60 + run, f16)
                    t32 = table.astype(np.float32)
                    adj = np.full((n, cap), -1, np.int32)
                    for v in range(n):
                        k = int(rng.integers(0, cap + 1))
                        ids = rng.permutation(n)[:k]
                        ids = ids[ids != v]
                        adj[v, np.sort(rng.permutation(cap)[: ids.shape[0]])] = ids
                    dist = np.full((n, cap), np.inf, np.float32)
                    vv, cc = np.nonzero(adj >= 0)
                    dist[vv, cc] = pair_dists(REF, t32, vv.astype(np.int32), adj[vv, cc], metric)
                    deg = (adj >= 0).sum(1).astype(np.int32)
                    ne = 4 * n * max(cap // 4, 1)
                    src = rng.integers(0, n - 20, ne).astype(np.int32)  # the last 20 rows are not affected
                    src[: ne // 4] = rng.integers(0, 6, ne // 4)  # six rows far over 2 cap
                    dst = rng.integers(0, n, ne).astype(np.int32)
                    dst[dst == src] = (src[dst == src] + 1) % n
                    w = pair_dists(REF, t32, src, dst, metric)
                    G = gb._LevelGraph(torch.arange(n), cap, selector="kernel")
                    G.alpha = alpha
                    G.adj, G.sim, G.deg = torch.from_numpy(adj.astype(np.int64)), torch.from_numpy(-dist), torch.from_numpy(deg.astype(np.int64))
                    G.add_links(torch.from_numpy(table), torch.from_numpy(src.astype(np.int64)), torch.from_numpy(dst.astype(np.int64)), torch.from_numpy(-w), metric)
                    a = (G.adj.numpy().astype(np.int32), np.ascontiguousarray(-G.sim.numpy()), G.deg.numpy().astype(np.int32))
                    b = ref_link(REF, table, adj, dist, deg, src, dst, w, metric, alpha)
                    c = _kernel(table, adj, dist, deg, src, dst, w, metric, alpha)
                    ok = same_bytes(a, b) and same_bytes(b, c) and b[0][n - 20 :].tobytes() == adj[n - 20 :].tobytes()
                    print(f"three-way metric={metric} f16={f16} cap={cap} alpha={alpha} n={n} edges={ne} full rows={int((c[2] == cap).sum())}: {'ok' if ok else 'MISMATCH'}", flush=True)
                    assert ok
                    run += 1


CASES["torch_form_agrees"] = case_torch_form_agrees


def _csr_equal(a, b):
    return (a.ntotal == b.ntotal and a.entry_point == b.entry_point and a.max_level == b.max_level and a.levels.tobytes() == b.levels.tobytes()
            and a.level_ptr.tobytes() == b.level_ptr.tobytes() and a.node_offsets.tobytes() == b.node_offsets.tobytes() and a.neighbors.tobytes() == b.neighbors.tobytes())


def case_builder_wiring():
    """build_graph_gpu and prune_preserving_hubs on CPU tensors with the oracle as candidate search, both with selector="kernel":
    linker="kernel" returns the CSR arrays of linker="torch" byte for byte, and the default is the torch linker."""
    import torch

    from leann_amd.gpu_graph_build import build_graph_gpu, prune_preserving_hubs
    from oracle import oracle as orc
    from tests.util import clustered, oracle_graph

    def oracle_search_fn(g, table, queries, ef, k):
        ids, dd, _ = orc.search(oracle_graph(g, g.d), queries.numpy(), k, ef=ef, beam=2, table=table.numpy())
        return torch.from_numpy(ids), torch.from_numpy(dd if g.metric_type == 0 else -dd)

    x = torch.from_numpy(clustered(500, 48, 5, n_centers=12, sigma=0.5))
    for metric in ("mips", "l2"):
        kw = dict(M=6, ef_construction=40, search_fn=oracle_search_fn, seed_nodes=128, selector="kernel")
        gt = build_graph_gpu(x, metric, linker="torch", **kw)
        gk = build_graph_gpu(x, metric, linker="kernel", **kw)
        gd = build_graph_gpu(x, metric, **kw)  # the default is the torch linker
        gk.validate()
        ok = _csr_equal(gt, gk) and _csr_equal(gt, gd)
        print(f"builder wiring {metric}: {gt.neighbors.shape[0]} links, max level-0 degree {gk.level0_degrees().max()}: {'ok' if ok else 'MISMATCH'}", flush=True)
        assert ok
        pt = prune_preserving_hubs(gt, x, M=6, m_low=3, hub_fraction=0.05, selector="kernel", linker="torch")
        pk = prune_preserving_hubs(gt, x, M=6, m_low=3, hub_fraction=0.05, selector="kernel", linker="kernel")
        ok = _csr_equal(pt, pk) and pt.neighbors.shape[0] < gt.neighbors.shape[0]
        print(f"pruning wiring {metric}: {pt.neighbors.shape[0]} links: {'ok' if ok else 'MISMATCH'}", flush=True)
        assert ok


CASES["builder_wiring"] = case_builder_wiring


def case_argument_checking():
    """Every argument the header rejects raises ValueError through _lib.check and launches nothing (adj / dist / deg keep their fill);
    ne == 0 and n == 0 are fine and write nothing; the workspace function; an unknown linker raises."""
    import pytest
    import torch

    from leann_amd import _lib
    from leann_amd.gpu_graph_build import _LevelGraph, build_graph_gpu, prune_preserving_hubs

    lib = _lib.load()
    n, cap, ne = 8, 4, 6
    table = np.zeros((n, 64), np.float32)
    src = np.array([0, 1, 2, 3, 4, 5], np.int32)
    dst = np.array([1, 2, 3, 4, 5, 6], np.int32)
    w = np.ones(ne, np.float32)
    need = int(lib.lm_graph_add_links_workspace_bytes(n, ne))
    assert need > 0
    ws = np.zeros(need + 8, np.uint8)
    good = dict(table=table.ctypes.data, dtype=0, dp=64, metric=0, n=n, cap=cap, ne=ne, alpha=1.0, ws=ws.ctypes.data, wsb=need, src=src.ctypes.data, dst=dst.ctypes.data,
                w=w.ctypes.data)

    def fresh():
        return np.full((n, cap), 0x6E6E6E6E, np.int32), np.full((n, cap), 7.5, np.float32), np.full(n, 0x6E6E6E6E, np.int32)

    def call(bufs, **over):
        a = dict(good, **over)
        adj, dist, deg = bufs
        return lib.lm_graph_add_links(a["table"], a["dtype"], a["dp"], a["metric"], a.get("adj", adj.ctypes.data), a.get("dist", dist.ctypes.data),
                                      a.get("deg", deg.ctypes.data), a["n"], a["cap"], a["src"], a["dst"], a["w"], a["ne"], a["alpha"], a["ws"], a["wsb"], None)

    def untouched(bufs):
        return all(x.tobytes() == y.tobytes() for x, y in zip(bufs, fresh()))

    bad = [dict(dp=48), dict(dp=0), dict(dp=-64), dict(dp=7 * 64), dict(dtype=2), dict(dtype=-1), dict(metric=5), dict(metric=-1), dict(cap=0), dict(cap=-2),
           dict(cap=_lib.SELECT_MAX_K // 2 + 1), dict(alpha=0.99), dict(alpha=0.0), dict(alpha=float("nan")), dict(alpha=float("inf")), dict(n=-1), dict(ne=-1),
           dict(n=(1 << 31)), dict(ne=(1 << 31)), dict(table=None), dict(adj=None), dict(dist=None), dict(deg=None), dict(src=None), dict(dst=None), dict(w=None),
           dict(ws=None), dict(ws=ws.ctypes.data + 1, wsb=need), dict(wsb=need - 1), dict(wsb=0)]
    for over in bad:
        bufs = fresh()
        with pytest.raises(ValueError):
            _lib.check(call(bufs, **over), "lm_graph_add_links")
        assert untouched(bufs), over
    for over in (dict(ne=0), dict(n=0), dict(ne=0, ws=None, wsb=0), dict(n=0, table=None, ws=None, wsb=0)):
        bufs = fresh()
        _lib.check(call(bufs, **over), "lm_graph_add_links")
        assert untouched(bufs), over
    # the workspace function: pure, 0 for what the call rejects, enough at any size, never decreasing
    f = lib.lm_graph_add_links_workspace_bytes
    assert f(n, ne) == need == f(n, ne) and f(-1, 5) == 0 and f(5, -1) == 0 and f(1 << 31, 5) == 0 and f(5, 1 << 31) == 0 and f(0, 5) == 0 and f(5, 0) == 0
    assert f(n + 1000, ne) >= need and f(n, ne + 1000) >= need and f((1 << 31) - 1, (1 << 31) - 1) > (1 << 33)
    bufs = fresh()
    _lib.check(call(bufs), "lm_graph_add_links")
    adj, dist, deg = bufs
    assert np.array_equal(adj[:6, 0], dst) and (adj[:6, 1:] == -1).all() and (dist[:6, 0] == 1.0).all() and np.isinf(dist[:6, 1:]).all() and (deg[:6] == 1).all()
    assert (adj[6:] == 0x6E6E6E6E).all() and (dist[6:] == 7.5).all() and (deg[6:] == 0x6E6E6E6E).all()
    print("argument checking: ok", flush=True)
    x = torch.zeros((10, 8))
    with pytest.raises(ValueError):
        build_graph_gpu(x, "mips", linker="bogus")
    with pytest.raises(ValueError):
        _LevelGraph(torch.arange(4), 4, linker="bogus")
    from leann_amd.hnsw_builder import build_hnsw

    g = build_hnsw(np.random.default_rng(0).standard_normal((50, 8)).astype(np.float32), "mips", M=4, ef_construction=10)
    with pytest.raises(ValueError):
        prune_preserving_hubs(g, torch.zeros((50, 8)), M=4, m_low=2, linker="bogus")
    print("linker checking: ok", flush=True)


CASES["argument_checking"] = case_argument_checking


if __name__ == "__main__":
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    _load(sys.argv[1])
    from tests.link_ref_util import load_ref

    REF = load_ref(sys.argv[2])
    import time

    import torch

    torch.set_num_threads(1)
    for name in (sys.argv[3:] or list(CASES)):
        t0 = time.time()
        CASES[name]()
        print(f"[case {name}: {time.time() - t0:.1f} s]", flush=True)
    print("ALL CASES OK")
