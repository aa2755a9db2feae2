"""Hub-preserving pruning scenarios run against libleann_mi355x_emul.so (tests/hip_emul/build_emul_lib.py: the product's kernels on the
CPU, a thread per lane) and the CPU restatement tests/prune_ref/lm_prune_ref.c.  Imported by tests/test_prune_kernel.py and runnable:
    python -m tests.emulated_prune_cases <path/to/libleann_mi355x_emul.so> <path/to/liblm_prune_ref.so> [case ...]
adj, dist (as bit patterns), deg, hubs and indeg are compared byte for byte."""
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


def _kernel(table, adj, m_low, n_hubs, metric, alpha, want_hubs=True, want_indeg=True):
    """lm_graph_prune_hubs through the ABI ('device' pointers are host pointers in the emulated world); outputs and workspace pre-filled
    with patterns the call must overwrite.  -> (adj, dist, deg, hubs, indeg)."""
    from leann_amd import _lib

    lib = _lib.load()
    table = np.ascontiguousarray(table)
    adj = np.ascontiguousarray(adj, np.int32)
    n, cap = adj.shape
    a, d, g = np.full((n, cap), 0x6E6E6E6E, np.int32), np.full((n, cap), 7.5, np.float32), np.full(n, 0x6E6E6E6E, np.int32)
    hubs, indeg = np.full(n_hubs, 0x6E6E6E6E, np.int32), np.full(n, 0x6E6E6E6E, np.int32)
    need = int(lib.lm_graph_prune_hubs_workspace_bytes(n, cap, m_low, n_hubs))
    ws = np.full(need // 8 + 1, 0xEEEEEEEEEEEEEEEE, np.uint64)
    before = adj.copy()
    rc = lib.lm_graph_prune_hubs(table.ctypes.data, _lib.DTYPE_F16 if table.dtype == np.float16 else _lib.DTYPE_F32, table.shape[1], metric, adj.ctypes.data, n, cap,
                                 m_low, n_hubs, alpha, a.ctypes.data, d.ctypes.data, g.ctypes.data, hubs.ctypes.data if want_hubs and n_hubs else None,
                                 indeg.ctypes.data if want_indeg else None, ws.ctypes.data, need, None)
    _lib.check(rc, "lm_graph_prune_hubs")
    assert adj.tobytes() == before.tobytes()  # the input is read only
    return a, d, g, hubs, indeg


def case_kernel_vs_restatement():
    """n in {1, 2, 1023, 1025, 3000} (the scan's tiles), cap in {1, 8, 64}, m_low in {1, 3, cap, cap + 5}, n_hubs in {0, 1, a cut in the
    middle of a group of equal in-degrees -- one that straddles row 1024 where there is one --, n}, the star at n = 3000, an all-empty
    graph, fp32 / fp16 tables with a NaN row and a zero row, both metrics, d_padded 64 and 384, alpha 1 and 1.2; some inputs twice."""
    from leann_amd import _lib
    from tests.prune_ref_util import EDGE_RUNS, check_star, differing, edge_case_adj, hubs_of_kind, in_degrees, ref_prune, table_for, usable_mask

    S = _lib.LINK_STAGE
    runs = EDGE_RUNS
    seen = {k: set() for k in ("n", "cap", "m_low", "hubs", "d", "metric", "f16", "alpha")}
    for run, (n, cap, m_low, kind, d, metric, f16, alpha, star, twice) in enumerate(runs):
        table = table_for(n, d, 100 + run, f16)
        adj = edge_case_adj(n, cap, 300 + run, S if star else 0)
        n_hubs = hubs_of_kind(kind, adj)
        got = _kernel(table, adj, m_low, n_hubs, metric, alpha)
        exp = ref_prune(REF, table, adj, m_low, n_hubs, metric, alpha)
        diff = differing(got, exp)
        ok = not diff
        # what the contract says about the result, independent of either implementation
        indeg = in_degrees(adj)
        ok = ok and np.array_equal(got[4], indeg)
        order = np.lexsort((np.arange(n), -indeg.astype(np.int64)))[:n_hubs]
        ok = ok and np.array_equal(got[3], order.astype(np.int32))
        valid = (got[0] >= 0) & (got[0] < n)
        ok = ok and np.array_equal(valid.sum(1), got[2]) and bool((got[0][~valid] == -1).all()) and bool(np.isinf(got[1][~valid]).all())
        um = usable_mask(adj)
        ok = ok and bool((got[2][(um.sum(1) == 0) & (indeg == 0)] == 0).all())  # no usable slot, in no list: the row stays empty
        if star:
            centre = check_star(adj, S)
            ok = ok and 1 <= got[2][7] <= cap
        if twice:
            ok = ok and not differing(_kernel(table, adj, m_low, n_hubs, metric, alpha), got)
            part = _kernel(table, adj, m_low, n_hubs, metric, alpha, want_hubs=False, want_indeg=False)  # the optional outputs left out
            ok = ok and not differing(part[:3], got[:3]) and bool((part[3] == 0x6E6E6E6E).all()) and bool((part[4] == 0x6E6E6E6E).all())
        print(f"prune n={n} cap={cap} m_low={m_low} n_hubs={n_hubs} ({kind}) d={d} metric={metric} f16={f16} alpha={alpha} max indeg={int(indeg.max(initial=0))}"
              f"{f' star={centre}' if star else ''} mean deg={got[2].mean():.2f}: {'ok' if ok else 'MISMATCH ' + ','.join(diff)}", flush=True)
        assert ok
        for k, v in zip(seen, (n, cap, "cap" if m_low == cap else "cap+5" if m_low == cap + 5 else m_low, kind, d, metric, f16, alpha)):
            seen[k].add(v)
    assert seen["n"] == {1, 2, 1023, 1025, 3000} and seen["cap"] == {1, 8, 64} and {1, 3, "cap", "cap+5"} <= seen["m_low"]
    assert seen["hubs"] == {"0", "1", "tie", "n"} and seen["d"] == {48, 384} and seen["metric"] == {0, 1} and seen["f16"] == {False, True} and seen["alpha"] == {1.0, 1.2}


CASES["kernel_vs_restatement"] = case_kernel_vs_restatement


def case_empty_graph_and_tie_straddle():
    """An all-empty graph (every in-degree 0: with n_hubs in the middle the hubs are the lowest ids, across the tile boundary; every
    output row empty), and the tie cut at n = 1025 checked for what it is: the group has members on both sides of row 1024."""
    from tests.prune_ref_util import differing, edge_case_adj, in_degrees, ref_prune, table_for, tie_cut

    n, cap = 1025, 8
    table = table_for(n, 48, 7, False)
    for fill in (-1, n + 2):
        adj = np.full((n, cap), fill, np.int32)
        for n_hubs in (0, 1024, 1025):
            got = _kernel(table, adj, 3, n_hubs, 0, 1.0)
            exp = ref_prune(REF, table, adj, 3, n_hubs, 0, 1.0)
            ok = not differing(got, exp) and bool((got[0] == -1).all()) and bool(np.isinf(got[1]).all()) and not got[2].any() and not got[4].any()
            ok = ok and np.array_equal(got[3], np.arange(n_hubs, dtype=np.int32))
            print(f"empty graph fill={fill} n_hubs={n_hubs}: {'ok' if ok else 'MISMATCH'}", flush=True)
            assert ok
    adj = edge_case_adj(n, cap, 11)
    indeg = in_degrees(adj)
    n_hubs = tie_cut(adj)
    order = np.lexsort((np.arange(n), -indeg.astype(np.int64)))
    T = indeg[order[n_hubs - 1]]
    members = np.nonzero(indeg == T)[0]
    taken = np.intersect1d(members, order[:n_hubs])
    assert indeg[order[n_hubs]] == T and members[0] < 1024 <= members[-1] and 0 < taken.shape[0] < members.shape[0]  # a cut inside a straddling group
    got = _kernel(table, adj, 3, n_hubs, 1, 1.0)
    ok = not differing(got, ref_prune(REF, table, adj, 3, n_hubs, 1, 1.0)) and np.array_equal(got[3], order[:n_hubs].astype(np.int32))
    print(f"tie cut n_hubs={n_hubs} T={T} group={members.shape[0]} taken={taken.shape[0]}: {'ok' if ok else 'MISMATCH'}", flush=True)
    assert ok


CASES["empty_graph_and_tie_straddle"] = case_empty_graph_and_tie_straddle


def _csr_equal(a, b):
    return (a.ntotal == b.ntotal and a.entry_point == b.entry_point and a.max_level == b.max_level and a.levels.tobytes() == b.levels.tobytes()
            and a.level_ptr.tobytes() == b.level_ptr.tobytes() and a.node_offsets.tobytes() == b.node_offsets.tobytes() and a.neighbors.tobytes() == b.neighbors.tobytes())


def case_python_wiring():
    """prune_level0_kernel and prune_preserving_hubs(pruner="kernel") on CPU tensors: the wrapper returns the restatement's arrays; the new
    graph's level-0 lists are the kernel's rows, upper levels and everything else copied; return_hubs; the default is the torch pruner and
    returns what pruner="torch" returns; an unknown pruner raises."""
    import pytest
    import torch

    from leann_amd import gpu_graph_build as gb
    from leann_amd.hnsw_builder import build_hnsw
    from tests.prune_ref_util import differing, ref_prune
    from tests.select_ref_util import pad64
    from tests.util import clustered

    x = clustered(400, 48, 5, n_centers=12, sigma=0.5)
    M, m_low = 6, 3
    for metric in ("mips", "l2"):
        g = build_hnsw(x, metric, M=M, ef_construction=40)
        cap = 2 * M
        n = g.ntotal
        p0 = g.node_offsets[:-1].astype(np.int64)
        beg, end = g.level_ptr[p0].astype(np.int64), g.level_ptr[p0 + 1].astype(np.int64)
        adj = np.full((n, cap), -1, np.int32)
        for v in range(n):
            adj[v, : end[v] - beg[v]] = g.neighbors[beg[v] : end[v]]
        nh = max(1, int(round(0.05 * n)))
        exp = ref_prune(REF, pad64(x), adj, m_low, nh, g.metric_type, 1.0)
        got = gb.prune_level0_kernel(torch.from_numpy(x), torch.from_numpy(adj), m_low, nh, g.metric_type, return_indeg=True)
        assert len(gb.prune_level0_kernel(torch.from_numpy(x), torch.from_numpy(adj), m_low, nh, g.metric_type)) == 4
        ok = not differing(tuple(t.numpy() for t in got), exp)
        pk, hubs = gb.prune_preserving_hubs(g, torch.from_numpy(x), M=M, m_low=m_low, hub_fraction=0.05, pruner="kernel", return_hubs=True)
        pk.validate()
        ok = ok and np.array_equal(hubs, exp[3].astype(np.int64)) and hubs.dtype == np.int64
        q0 = pk.node_offsets[:-1].astype(np.int64)
        for v in range(n):
            row = pk.neighbors[int(pk.level_ptr[q0[v]]) : int(pk.level_ptr[q0[v] + 1])]
            ok = ok and np.array_equal(row, exp[0][v, : exp[2][v]])
        ok = ok and pk.levels.tobytes() == g.levels.tobytes() and pk.entry_point == g.entry_point and pk.neighbors.shape[0] < g.neighbors.shape[0]
        up = np.nonzero(g.levels > 1)[0]
        for i in up:  # upper levels copied
            for l in range(1, int(g.levels[i])):
                a = g.neighbors[int(g.level_ptr[int(g.node_offsets[i]) + l]) : int(g.level_ptr[int(g.node_offsets[i]) + l + 1])]
                b = pk.neighbors[int(pk.level_ptr[int(pk.node_offsets[i]) + l]) : int(pk.level_ptr[int(pk.node_offsets[i]) + l + 1])]
                ok = ok and np.array_equal(a, b)
        pd = gb.prune_preserving_hubs(g, torch.from_numpy(x), M=M, m_low=m_low, hub_fraction=0.05)
        pt, th = gb.prune_preserving_hubs(g, torch.from_numpy(x), M=M, m_low=m_low, hub_fraction=0.05, pruner="torch", return_hubs=True)
        ok = ok and _csr_equal(pd, pt) and th.shape[0] == nh
        print(f"python wiring {metric}: {pk.neighbors.shape[0]} links (torch form {pt.neighbors.shape[0]}), {up.shape[0]} upper nodes: {'ok' if ok else 'MISMATCH'}", flush=True)
        assert ok
        with pytest.raises(ValueError):
            gb.prune_preserving_hubs(g, torch.from_numpy(x), M=M, m_low=m_low, pruner="bogus")
        same, none = gb.prune_preserving_hubs(g, torch.from_numpy(x), M=M, m_low=2 * M, pruner="kernel", return_hubs=True)
        assert same is g and none.shape == (0,)


CASES["python_wiring"] = case_python_wiring


def case_argument_checking():
    """Every argument the header rejects raises ValueError through _lib.check and launches nothing (the outputs keep their fill); n == 0
    is fine and writes nothing; the workspace function."""
    import pytest

    from leann_amd import _lib

    lib = _lib.load()
    n, cap, m_low, nh = 8, 4, 2, 2
    table = np.zeros((n, 64), np.float32)
    adj = np.full((n, cap), -1, np.int32)
    adj[:, 0] = (np.arange(n) + 1) % n
    f = lib.lm_graph_prune_hubs_workspace_bytes
    need = int(f(n, cap, m_low, nh))
    assert need > 0
    ws = np.zeros(need // 8 + 2, np.uint64)
    good = dict(table=table.ctypes.data, dtype=0, dp=64, metric=0, adj_in=adj.ctypes.data, n=n, cap=cap, m_low=m_low, nh=nh, alpha=1.0, ws=ws.ctypes.data, wsb=need)

    def fresh():
        return (np.full((n, cap), 0x6E6E6E6E, np.int32), np.full((n, cap), 7.5, np.float32), np.full(n, 0x6E6E6E6E, np.int32), np.full(n, 0x6E6E6E6E, np.int32),
                np.full(n, 0x6E6E6E6E, np.int32))

    def call(bufs, **over):
        a = dict(good, **over)
        ao, do, go, hubs, indeg = bufs
        return lib.lm_graph_prune_hubs(a["table"], a["dtype"], a["dp"], a["metric"], a["adj_in"], a["n"], a["cap"], a["m_low"], a["nh"], a["alpha"],
                                       a.get("adj", ao.ctypes.data), a.get("dist", do.ctypes.data), a.get("deg", go.ctypes.data), hubs.ctypes.data, indeg.ctypes.data,
                                       a["ws"], a["wsb"], None)

    def untouched(bufs):
        return all(x.tobytes() == y.tobytes() for x, y in zip(bufs, fresh()))

    big = (1 << 31) // cap + 1  # n * cap > INT32_MAX
    bad = [dict(dp=48), dict(dp=0), dict(dp=-64), dict(dp=7 * 64), dict(dtype=2), dict(dtype=-1), dict(metric=5), dict(metric=-1), dict(cap=0), dict(cap=-2),
           dict(cap=_lib.SELECT_MAX_K // 2 + 1), dict(alpha=0.99), dict(alpha=0.0), dict(alpha=float("nan")), dict(alpha=float("inf")), dict(m_low=0), dict(m_low=-3),
           dict(nh=-1), dict(nh=n + 1), dict(n=-1), dict(n=big, nh=0), dict(n=1 << 40, nh=0), dict(n=(1 << 29) - 1, cap=4, m_low=4, nh=0),  # ne = 2 n cap > INT32_MAX
           dict(table=None), dict(adj_in=None), dict(adj=None), dict(dist=None), dict(deg=None), dict(ws=None), dict(adj=adj.ctypes.data),
           dict(ws=ws.ctypes.data + 4), dict(ws=ws.ctypes.data + 1), dict(wsb=need - 1), dict(wsb=0)]
    for over in bad:
        bufs = fresh()
        with pytest.raises(ValueError):
            _lib.check(call(bufs, **over), "lm_graph_prune_hubs")
        assert untouched(bufs), over
    for over in (dict(n=0, nh=0), dict(n=0, nh=0, table=None, adj_in=None, adj=None, dist=None, deg=None, ws=None, wsb=0)):
        bufs = fresh()
        _lib.check(call(bufs, **over), "lm_graph_prune_hubs")
        assert untouched(bufs), over
    # the workspace function: pure, 0 for what the call rejects and for n == 0, covers the inner link insertion, never decreasing
    ne = 2 * (nh * cap + (n - nh) * m_low)
    assert f(n, cap, m_low, nh) == need and need >= int(lib.lm_graph_add_links_workspace_bytes(n, ne)) + 3 * 4 * ne + 8 * n
    assert f(0, cap, m_low, 0) == 0 and f(-1, cap, m_low, 0) == 0 and f(n, 0, m_low, nh) == 0 and f(n, _lib.SELECT_MAX_K // 2 + 1, m_low, nh) == 0
    assert f(n, cap, 0, nh) == 0 and f(n, cap, m_low, -1) == 0 and f(n, cap, m_low, n + 1) == 0 and f(big, cap, m_low, 0) == 0 and f((1 << 29) - 1, 4, 4, 0) == 0
    assert f(n, cap, m_low + 50, nh) == f(n, cap, cap, nh) >= need and f(n + 1000, cap, m_low, nh) >= need and f(n, cap, m_low, n) >= need
    bufs = fresh()
    _lib.check(call(bufs), "lm_graph_prune_hubs")
    ao, do, go, hubs, indeg = bufs
    # a ring v -> v + 1 over all-zero vectors: every in-degree 1, hubs 0 and 1; every row ends with its successor and its predecessor
    assert (indeg == 1).all() and hubs[:nh].tolist() == [0, 1] and (hubs[nh:] == 0x6E6E6E6E).all() and (go == 2).all()
    assert all(sorted(ao[v, :2].tolist()) == sorted([(v + 1) % n, (v - 1) % n]) for v in range(n)) and (ao[:, 2:] == -1).all() and (do[:, :2] == 0).all()
    print("argument checking: ok", flush=True)


CASES["argument_checking"] = case_argument_checking


if __name__ == "__main__":
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    _load(sys.argv[1])
    from tests.prune_ref_util import load_ref

    REF = load_ref(sys.argv[2])
    import time

    import torch

    torch.set_num_threads(1)
    for name in (sys.argv[3:] or list(CASES)):
        t0 = time.time()
        CASES[name]()
        print(f"[case {name}: {time.time() - t0:.1f} s]", flush=True)
    print("ALL CASES OK")
