"""Neighbour-selection scenarios run against libleann_mi355x_emul.so (tests/hip_emul/build_emul_lib.py: the product's kernels on the CPU,
a thread per lane) and the CPU restatement tests/select_ref/lm_select_ref.c.  Imported by tests/test_select_neighbors.py and runnable:
    python -m tests.emulated_select_cases <path/to/libleann_mi355x_emul.so> <path/to/liblm_select_ref.so> [case ...]
Keep masks are compared byte for byte."""
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


def _kernel(table, cand, dist, m, metric, alpha):
    """lm_select_neighbors through the ABI on numpy arrays ('device' pointers are host pointers in the emulated world)."""
    from leann_amd import _lib

    table = np.ascontiguousarray(table)
    cand = np.ascontiguousarray(cand, np.int32)
    dist = np.ascontiguousarray(dist, np.float32)
    n, K = cand.shape
    keep = np.full((n, K), 0xEE, np.uint8)  # the kernel must write every byte
    rc = _lib.load().lm_select_neighbors(table.ctypes.data, _lib.DTYPE_F16 if table.dtype == np.float16 else _lib.DTYPE_F32, table.shape[0], table.shape[1],
                                         metric, cand.ctypes.data, dist.ctypes.data, n, K, m, alpha, keep.ctypes.data, None)
    _lib.check(rc, "lm_select_neighbors")
    return keep


def _table(N, d, seed, f16):
    from tests.select_ref_util import pad64
    from tests.util import clustered

    x = clustered(N, d, seed, n_centers=8, sigma=0.5)
    nd = N // 6
    x[:nd] = x[nd : 2 * nd]  # duplicate vectors: exact ties
    return pad64(x.astype(np.float16) if f16 else x)


def case_kernel_vs_restatement():
    """Both metrics, fp32 / fp16 tables, alpha in {1, 1.2, 1.5}, d in {48 -> 64, 96 -> 128, 384}, (K, m) from (1, 1) to the exported limit,
    row counts that are no multiple of the 16 rows a workgroup holds; rows from tests.select_ref_util.awkward_rows."""
    from leann_amd import _lib
    from tests.select_ref_util import awkward_rows, ref_select

    shapes = [(1, 1, 203), (7, 3, 301), (64, 12, 150), (128, 64, 37), (193, 32, 29), (_lib.SELECT_MAX_K, 64, 9)]
    combos = [(metric, f16, alpha) for metric in (0, 1) for f16 in (False, True) for alpha in (1.0, 1.2, 1.5)]
    seen = set()
    run = 0
    for si, (K, m, n) in enumerate(shapes):
        # small shapes: the whole metric x dtype x alpha product at every d; large ones (the emulation runs a thread per lane): four
        # combinations each, rotated so that every value of every factor meets a large shape
        small = K <= 64
        for di, d in enumerate((48, 96, 384)):
            pick = combos if small and d != 384 else [combos[(3 * si + 5 * di + 7 * t) % len(combos)] for t in range(4)]
            for metric, f16, alpha in pick:
                table = _table(max(K + 7, 300), d, 100 + run, f16)
                cand, dist = awkward_rows(table.astype(np.float32), n, K, metric, 200 + run)
                got = _kernel(table, cand, dist, m, metric, alpha)
                exp = ref_select(REF, table, cand, dist, m, metric, alpha)
                ok = np.array_equal(got, exp)
                if run % 7 == 0:  # the same input again: the same bytes
                    ok = ok and np.array_equal(_kernel(table, cand, dist, m, metric, alpha), got)
                valid = (cand >= 0) & (cand < table.shape[0])
                ok = ok and not bool((got[~valid] != 0).any()) and int(got.sum(1).max()) <= m and set(np.unique(got).tolist()) <= {0, 1}
                print(f"select K={K} m={m} n={n} d={d} metric={metric} f16={f16} alpha={alpha} kept/row={got.sum() / n:.2f}: {'ok' if ok else 'MISMATCH'}", flush=True)
                assert ok
                seen.add((metric, f16, alpha, d))
                run += 1
    assert {s[:3] for s in seen} == set(combos) and {s[3] for s in seen} == {48, 96, 384}


CASES["kernel_vs_restatement"] = case_kernel_vs_restatement


def _integer_rows(N, d, n, K, metric, seed):
    """Vectors with small integer entries (|x| <= 3): every inner product and squared distance is an exact integer in fp32 whatever the
    summation order (|sum| <= 96 * 36 < 2^24), so torch's matmul, the oracle's reduction and the kernel's agree to the bit."""
    from tests.select_ref_util import internal_dist

    rng = np.random.default_rng(seed)
    x = rng.integers(-3, 4, (N, d)).astype(np.float32)
    base = rng.integers(0, N, n)
    cand = np.stack([rng.permutation(N)[:K] for _ in range(n)]).astype(np.int32)
    rows = rng.random(n) < 0.3
    cand[rows, K // 2] = cand[rows, 0]  # duplicate ids inside a row
    dist = internal_dist(x, base, cand, metric)
    o = np.argsort(dist, axis=1, kind="stable")
    cand, dist = np.take_along_axis(cand, o, 1), np.take_along_axis(dist, o, 1)
    empty = (np.arange(K)[None, :] >= rng.integers(1, K + 1, n)[:, None]) | (rng.random((n, K)) < 0.05)
    cand[empty] = -1
    dist[empty] = np.float32(np.inf)
    return x, cand, dist


def case_three_way_on_exact_arithmetic():
    """alpha = 1, integer-valued vectors: gpu_graph_build._select_heuristic_scan (fp32 on CPU tensors), the C restatement and the kernel
    return the same mask.  Ties are everywhere in such data, so this also pins the `<=` of the rule to the existing definition."""
    import torch

    from leann_amd import gpu_graph_build as gb
    from tests.select_ref_util import pad64, ref_select

    for metric in (0, 1):
        for (N, d, n, K, m) in ((300, 48, 210, 24, 8), (200, 96, 101, 64, 16), (120, 16, 150, 32, 32), (64, 8, 99, 12, 3)):
            x, cand, dist = _integer_rows(N, d, n, K, metric, 7 * d + metric)
            a = gb._select_heuristic_scan(torch.from_numpy(x), torch.from_numpy(cand.astype(np.int64)), torch.from_numpy(-dist), m, metric).numpy().astype(np.uint8)
            for f16 in (False, True):  # small integers are exact in fp16 as well
                table = pad64(x.astype(np.float16) if f16 else x)
                b = ref_select(REF, table, cand, dist, m, metric, 1.0)
                c = _kernel(table, cand, dist, m, metric, 1.0)
                ok = np.array_equal(a, b) and np.array_equal(b, c)
                print(f"three-way metric={metric} N={N} d={d} K={K} m={m} f16={f16} kept/row={a.sum() / n:.2f}: {'ok' if ok else 'MISMATCH'}", flush=True)
                assert ok
            # the data does hold ties at the rule's comparison (else this case would not pin `<=` against `<`)
            v = x[np.clip(cand, 0, None)]
            gram = np.einsum("rid,rjd->rij", v, v)  # exact integers
            sq = (v * v).sum(-1)
            pd = sq[:, :, None] + sq[:, None, :] - 2 * gram if metric == 1 else -gram
            ties = int(((pd == dist[:, :, None]) & (cand[:, :, None] >= 0) & (cand[:, None, :] >= 0) & (np.arange(K)[None, :, None] > np.arange(K)[None, None, :])).sum())
            assert ties > 0
            # and the wrapper the builder calls returns the same mask as a bool tensor
            w = gb.select_neighbors_kernel(torch.from_numpy(x), torch.from_numpy(cand.astype(np.int64)), torch.from_numpy(-dist), m, metric, 1.0)
            assert w.dtype == torch.bool and np.array_equal(w.numpy().astype(np.uint8), a)


CASES["three_way_on_exact_arithmetic"] = case_three_way_on_exact_arithmetic


def _csr_equal(a, b):
    return (a.ntotal == b.ntotal and a.entry_point == b.entry_point and a.max_level == b.max_level and np.array_equal(a.levels, b.levels)
            and np.array_equal(a.level_ptr, b.level_ptr) and np.array_equal(a.node_offsets, b.node_offsets) and np.array_equal(a.neighbors, b.neighbors))


def case_builder_wiring():
    """build_graph_gpu and prune_preserving_hubs on CPU tensors with the oracle as candidate search, integer-valued data (exact arithmetic:
    both selectors see the same masks, hence every later step is the same): selector="kernel" returns the CSR arrays of selector="torch"."""
    import torch

    from leann_amd.gpu_graph_build import build_graph_gpu, prune_preserving_hubs
    from oracle import oracle as orc
    from tests.util import oracle_graph

    def oracle_search_fn(g, table, queries, ef, k):
        ids, dd, _ = orc.search(oracle_graph(g, g.d), queries.numpy(), k, ef=ef, beam=2, table=table.numpy())
        return torch.from_numpy(ids), torch.from_numpy(dd if g.metric_type == 0 else -dd)

    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.integers(-3, 4, (1500, 48)).astype(np.float32))
    for metric in ("mips", "l2"):
        kw = dict(M=8, ef_construction=40, search_fn=oracle_search_fn, seed_nodes=256)
        gt = build_graph_gpu(x, metric, selector="torch", **kw)
        gk = build_graph_gpu(x, metric, selector="kernel", **kw)
        gd = build_graph_gpu(x, metric, **kw)  # the default is the torch selector
        gk.validate()
        ok = _csr_equal(gt, gk) and _csr_equal(gt, gd)
        print(f"builder wiring {metric}: {gt.neighbors.shape[0]} links: {'ok' if ok else 'MISMATCH'}", flush=True)
        assert ok
        pt = prune_preserving_hubs(gt, x, M=8, m_low=4, hub_fraction=0.05, selector="torch")
        pk = prune_preserving_hubs(gt, x, M=8, m_low=4, hub_fraction=0.05, selector="kernel")
        ok = _csr_equal(pt, pk) and pt.neighbors.shape[0] < gt.neighbors.shape[0]
        print(f"pruning wiring {metric}: {pt.neighbors.shape[0]} links: {'ok' if ok else 'MISMATCH'}", flush=True)
        assert ok


CASES["builder_wiring"] = case_builder_wiring


def case_argument_checking():
    """Every argument the header rejects raises ValueError through _lib.check and launches nothing (the keep buffer keeps its fill);
    n = 0 is fine; an unknown selector raises."""
    import pytest
    import torch

    from leann_amd import _lib
    from leann_amd.gpu_graph_build import _LevelGraph, build_graph_gpu, prune_preserving_hubs

    lib = _lib.load()
    table = np.zeros((8, 64), np.float32)
    cand = np.zeros((4, 4), np.int32)
    dist = np.zeros((4, 4), np.float32)
    good = dict(dtype=0, ntable=8, dp=64, metric=0, n=4, K=4, m=2, alpha=1.0)

    def call(keep, **over):
        a = dict(good, **over)
        return lib.lm_select_neighbors(table.ctypes.data, a["dtype"], a["ntable"], a["dp"], a["metric"], cand.ctypes.data, dist.ctypes.data, a["n"], a["K"], a["m"],
                                       a["alpha"], keep.ctypes.data, None)

    keep = np.full((4, 4), 0xEE, np.uint8)
    bad = [dict(dp=48), dict(dp=0), dict(dp=7 * 64), dict(K=0), dict(K=-3), dict(K=_lib.SELECT_MAX_K + 1), dict(m=0), dict(m=-1), dict(alpha=0.99), dict(alpha=0.0),
           dict(alpha=float("nan")), dict(alpha=float("inf")), dict(n=-1), dict(dtype=2), dict(metric=5)]
    for over in bad:
        with pytest.raises(ValueError):
            _lib.check(call(keep, **over), "lm_select_neighbors")
        assert (keep == 0xEE).all(), over
    _lib.check(call(keep, n=0))
    assert (keep == 0xEE).all()
    _lib.check(call(keep))
    assert set(np.unique(keep).tolist()) <= {0, 1}
    print("argument checking: ok", flush=True)
    x = torch.zeros((10, 8))
    with pytest.raises(ValueError):
        build_graph_gpu(x, "mips", selector="bogus")
    with pytest.raises(ValueError):
        _LevelGraph(torch.arange(4), 4, selector="bogus")
    from leann_amd.hnsw_builder import build_hnsw

    g = build_hnsw(np.random.default_rng(0).standard_normal((50, 8)).astype(np.float32), "mips", M=4, ef_construction=10)
    with pytest.raises(ValueError):
        prune_preserving_hubs(g, torch.zeros((50, 8)), M=4, m_low=2, selector="bogus")
    print("selector checking: ok", flush=True)


CASES["argument_checking"] = case_argument_checking


if __name__ == "__main__":
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    _load(sys.argv[1])
    from tests.select_ref_util import load_ref

    REF = load_ref(sys.argv[2])
    import time

    import torch

    torch.set_num_threads(1)
    for name in (sys.argv[3:] or list(CASES)):
        t0 = time.time()
        CASES[name]()
        print(f"[case {name}: {time.time() - t0:.1f} s]", flush=True)
    print("ALL CASES OK")
