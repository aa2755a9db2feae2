"""Exact-search scenarios run against libleann_mi355x_emul.so (tests/hip_emul/build_emul_lib.py: the product's kernels on the CPU, a thread
per lane) and the oracle's bruteforce_topk.  Imported by tests/test_exact_search.py and runnable:
    python -m tests.emulated_exact_cases <path/to/libleann_mi355x_emul.so> [case ...]
Labels are compared for equality, distances bit for bit."""
import sys
from pathlib import Path

import numpy as np

CASES = {}


def _load(lib_path: str):
    from leann_amd import _lib

    _lib.LIB_PATH = Path(lib_path)
    _lib._lib = None
    return _lib.load()


def _check(tag, table, q, k, metric, mask=None, stray=False):
    from leann_amd import _lib
    from tests import gpu_exact_util as xu

    words = None if mask is None else xu.bitmap(mask, stray)
    rc, L, D, guards = xu.exact_host(_lib.load(), table, q, k, metric, words)
    el, ed = xu.expected(table, q, k, metric, mask)
    ok = rc == 0 and guards and xu.same(L, D, el, ed)
    print(f"exact {tag} n={table.shape[0]} dp={table.shape[1]} nq={q.shape[0]} k={k} metric={metric} f16={table.dtype == np.float16} "
          f"slices={xu.plan(table.shape[0], q.shape[0])[0]}: {'ok' if ok else 'MISMATCH'}", flush=True)
    assert ok
    return L, D


def case_kernel_vs_oracle():
    """Both metrics, fp32 / fp16 tables, d in {48 -> 64, 96 -> 128, 384}, k in {1, 10, LM_EXACT_MAX_K}, nq in {1, 5}, and the three slicing regimes
    of the policy: one slice (<= 1024 rows), two (1025 .. 2048), many with a short last one (2500 rows: 3 slices of 864, 864, 772).  The full
    product at d = 48, a rotation through it at the wider rows (the emulation runs a thread per lane)."""
    from leann_amd import _lib
    from tests import gpu_exact_util as xu

    assert xu.plan(700, 1) == (1, 704) and xu.plan(1500, 5) == (2, 768) and xu.plan(2500, 1) == (3, 864)
    combos = [(metric, f16, k, nq) for metric in (0, 1) for f16 in (False, True) for k in (1, 10, _lib.EXACT_MAX_K) for nq in (1, 5)]
    run = 0
    seen = set()
    for ni, n in enumerate((700, 1500, 2500)):
        for di, d in enumerate((48, 96, 384)):
            pick = combos if d == 48 and n != 2500 else [combos[(5 * ni + 7 * di + 11 * t) % len(combos)] for t in range(6)]
            for metric, f16, k, nq in pick:
                table, q = xu.gauss_case(n, d, nq, 300 + run, f16)
                L, D = _check("gauss", table, q, k, metric)
                if run % 9 == 0:  # the same input again: the same bits
                    L2, D2 = _check("again", table, q, k, metric)
                    assert xu.same(L2, D2, L, D)
                seen.add((metric, f16, k, nq, d, xu.plan(n, nq)[0]))
                run += 1
    for pos, vals in enumerate(((0, 1), (False, True), (1, 10, _lib.EXACT_MAX_K), (1, 5), (48, 96, 384), (1, 2, 3))):
        assert {s[pos] for s in seen} == set(vals), (pos, vals)


CASES["kernel_vs_oracle"] = case_kernel_vs_oracle


def case_small_tables_and_ties():
    """Fewer rows than k (the -1 / inf fills), ntable in {0, 1, k - 1, k, k + 1}, a query tile and one more, NaN and exact-zero rows, integer
    rows whose equal distances straddle the slices and the k-th rank."""
    from tests import gpu_exact_util as xu

    for metric in (0, 1):
        for n in (0, 1, 9, 10, 11, 65):
            table, q = xu.gauss_case(n, 48, 3, 40 + n, n % 2 == 1)
            if n == 0:
                table = np.zeros((0, 64), np.float32)
            _check("small", table, q, 10, metric)
        table, q = xu.gauss_case(333, 96, 9, 77, False)  # nq = one more than a tile of eight
        _check("tile+1", table, q, 10, metric)
        table, q = xu.gauss_case(200, 48, 2, 78, False)
        table[17, 3] = np.nan
        table[50] = 0.0  # inner product exactly 0 -> the key's +0, returned as -0.0 for ip
        table[120] = -table[50]
        L, D = _check("nan/zero", table, q, 200, metric)
        assert L[0, -1] == 17 and np.isinf(D[0, -1])  # NaN ranks as +inf: last
        if metric == 0:
            z = int(np.flatnonzero(L[0] == 50)[0])
            assert D[0, z].view(np.uint32) == 0x80000000
        for f16 in (False, True):
            table, q = xu.integer_case(2500, 48, 5, 90 + metric, f16)
            el, ed = xu.expected(table, q, 10, metric)
            far = xu.expected(table, q, 11, metric)[1]
            assert (far[:, 9] == far[:, 10]).any()  # a tie between ranks k and k + 1
            rows = xu.plan(2500, 5)[1]
            tie = (ed[:, :-1] == ed[:, 1:]) & (el[:, :-1] // rows != el[:, 1:] // rows)
            assert tie.any()  # and tie pairs whose ids lie in different slices
            _check("ties", table, q, 10, metric)


CASES["small_tables_and_ties"] = case_small_tables_and_ties


def case_allow_list():
    """A random half, fewer than k rows allowed, nobody allowed, ntable % 32 != 0 with the stray high bits of the last word set."""
    from tests import gpu_exact_util as xu

    rng = np.random.default_rng(3)
    for metric in (0, 1):
        for n, f16 in ((1500, False), (333, True)):
            table, q = xu.gauss_case(n, 48, 3, 50 + n + metric, f16)
            _check("half", table, q, 10, metric, rng.random(n) < 0.5)
            few = np.zeros(n, bool)
            few[rng.permutation(n)[:6]] = True
            L, _ = _check("few", table, q, 10, metric, few)
            assert (L[:, 6:] == -1).all() and (L[:, :6] >= 0).all()
            L, _ = _check("none", table, q, 10, metric, np.zeros(n, bool))
            assert (L == -1).all()
            _check("stray", table, q, 10, metric, rng.random(n) < 0.5, stray=True)
            _check("all+stray", table, q, n if n < 256 else 256, metric, np.ones(n, bool), stray=True)


CASES["allow_list"] = case_allow_list


def case_argument_checking():
    """Everything the header rejects returns LM_EINVAL and touches no buffer (no device call: outputs and workspace keep their fill); nq == 0 is
    fine and writes nothing."""
    from leann_amd import _lib
    from tests import gpu_exact_util as xu

    lib = _lib.load()
    table, q = xu.gauss_case(40, 64, 2, 1, False)
    bad = [dict(d_padded=48), dict(d_padded=0), dict(d_padded=7 * 64), dict(d_padded=-64), dict(dtype=2), dict(dtype=-1), dict(metric=2), dict(metric=-1), dict(k=0),
           dict(k=-1), dict(k=_lib.EXACT_MAX_K + 1), dict(nq=-1), dict(ntable=-1), dict(ntable=2**31), dict(ws_short=1)]
    for over in bad:
        a = dict(k=10, metric=0)
        a.update(over)
        rc, _, _, untouched = xu.exact_host(lib, table, q, a.pop("k"), a.pop("metric"), **a)
        assert rc == _lib.LM_EINVAL and untouched, over
        try:
            _lib.check(rc, "lm_exact_search")
        except ValueError:
            pass
        else:
            raise AssertionError("LM_EINVAL must map to ValueError")
    nb = lib.lm_exact_search_workspace_bytes(40, 2, 10)
    ws, D, L = np.zeros(max(nb, 8), np.uint8), np.zeros((2, 10), np.float32), np.zeros((2, 10), np.int64)
    good = [table.ctypes.data, 0, 40, 64, 0, q.ctypes.data, 2, 10, None, D.ctypes.data, L.ctypes.data, ws.ctypes.data, nb, None]
    for pos in (0, 5, 9, 10, 11):  # a NULL buffer where one is needed
        args = list(good)
        args[pos] = None
        assert lib.lm_exact_search(*args) == _lib.LM_EINVAL, pos
    assert lib.lm_exact_search(*good) == 0
    rc, _, _, untouched = xu.exact_host(lib, table, q, 10, 0, nq=0)
    assert rc == 0 and untouched
    assert lib.lm_exact_search_workspace_bytes(40, 2, 10) == 1 * 2 * 10 * 8 and lib.lm_exact_search_workspace_bytes(2500, 1, 7) == 3 * 7 * 8
    print("argument checking: ok", flush=True)


CASES["argument_checking"] = case_argument_checking


def case_wiring():
    """Mi355xIndex.search_exact (fp32 host table and a borrowed fp16 one, mask and id-array allow-lists, LM_ESTATE without a table),
    exact.exact_topk_kernel, and the backend's exact=True / allowed_ids on a bundle built with is_recompute=False."""
    import tempfile

    import torch

    from leann_amd._compat import BACKEND_REGISTRY
    from leann_amd.backend import write_leann_bundle
    from leann_amd.exact import exact_topk_kernel
    from leann_amd.hnsw_builder import build_hnsw
    from leann_amd.index import Mi355xIndex, allow_bitmap
    from tests import gpu_exact_util as xu
    from tests.util import clustered

    n, d = 600, 48
    x = clustered(n, d, 5, n_centers=8, sigma=0.5)
    q = x[:4] + 0.01
    rng = np.random.default_rng(8)
    mask = rng.random(n) < 0.3
    assert np.array_equal(allow_bitmap(mask, n), xu.bitmap(mask)) and np.array_equal(allow_bitmap(np.flatnonzero(mask), n), xu.bitmap(mask))
    for bad in (np.array([n]), np.array([-1]), np.zeros(n + 1, bool)):
        try:
            allow_bitmap(bad, n)
        except ValueError:
            continue
        raise AssertionError("allow_bitmap must reject it")
    for metric in ("mips", "l2"):
        m = 0 if metric == "mips" else 1
        g = build_hnsw(x, metric, M=6, ef_construction=30)
        idx = Mi355xIndex.from_csr(g)
        try:
            idx.search_exact(q, 5)
        except RuntimeError:  # LM_ESTATE: no table yet
            pass
        else:
            raise AssertionError("search_exact without a table must raise")
        idx.attach_table(x)
        prm = idx.make_params(ef=32, beam=2, recompute=False)
        before = idx.search(q, 5, prm)
        D, L = idx.search_exact(q, 7)
        assert xu.same(L, D, *xu.expected(xu.pad64(x), xu.pad64(q), 7, m))
        for allowed in (mask, np.flatnonzero(mask)):
            D, L = idx.search_exact(q, 7, allowed=allowed)
            assert xu.same(L, D, *xu.expected(xu.pad64(x), xu.pad64(q), 7, m, mask))
        after = idx.search(q, 5, prm)
        assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
        h = torch.from_numpy(xu.pad64(x.astype(np.float16)))  # "device" tensor of the emulated world
        idx._lib.lm_index_attach_table(idx._h, h.data_ptr(), 1, n, d, 1)
        D, L = idx.search_exact(q, 7, allowed=mask)
        assert xu.same(L, D, *xu.expected(xu.pad64(x.astype(np.float16)), xu.pad64(q), 7, m, mask))
        idx.close()
        v, i = exact_topk_kernel(torch.from_numpy(q), torch.from_numpy(x), 9, metric)
        el, ed = xu.expected(xu.pad64(x), xu.pad64(q), 9, m)
        assert tuple(v.shape) == (4, 9) and v.dtype == torch.float32 and i.dtype == torch.int64 and xu.same(i.numpy(), v.numpy(), el, ed)
        print(f"index / exact_topk_kernel wiring {metric}: ok", flush=True)
    with tempfile.TemporaryDirectory() as td:
        p = str(Path(td) / "full.leann")
        write_leann_bundle(p, [f"passage {i}" for i in range(n)], x, "sentence-transformers/all-MiniLM-L6-v2", distance_metric="l2", M=6, efConstruction=30, is_recompute=False)
        s = BACKEND_REGISTRY["mi355x"].searcher(p)
        r = s.search(q, 6, recompute_embeddings=False, exact=True)
        el, ed = xu.expected(xu.pad64(x), xu.pad64(q), 6, 1)
        assert r["labels"] == [[str(int(v)) for v in row] for row in el] and xu.same(el, r["distances"], el, ed)
        few = np.flatnonzero(mask)[:4]
        r = s.search(q, 6, recompute_embeddings=False, exact=True, allowed_ids=[int(v) for v in few])
        fm = np.zeros(n, bool)
        fm[few] = True
        el, ed = xu.expected(xu.pad64(x), xu.pad64(q), 6, 1, fm)
        assert r["labels"] == [[str(int(v)) for v in row] for row in el] and r["labels"][0][4:] == ["-1", "-1"] and xu.same(el, r["distances"], el, ed)
        for kw, exc in ((dict(recompute_embeddings=False, allowed_ids=[1]), ValueError), (dict(recompute_embeddings=True, zmq_port=5555, exact=True), RuntimeError)):
            try:
                s.search(q, 6, **kw)
            except exc as ex:
                assert exc is ValueError or "Recompute is required" in str(ex)
            else:
                raise AssertionError(f"{kw} must raise {exc.__name__}")
        s.cleanup()
        p2 = str(Path(td) / "pruned.leann")
        write_leann_bundle(p2, [f"passage {i}" for i in range(n)], x, "sentence-transformers/all-MiniLM-L6-v2", distance_metric="l2", M=6, efConstruction=30)
        s = BACKEND_REGISTRY["mi355x"].searcher(p2)
        try:
            s.search(q, 6, recompute_embeddings=False, exact=True)
        except RuntimeError as ex:
            assert "Recompute is required" in str(ex)
        else:
            raise AssertionError("exact=True on a pruned index must raise")
        s.cleanup()
    print("backend wiring: ok", flush=True)


CASES["wiring"] = case_wiring


if __name__ == "__main__":
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    _load(sys.argv[1])
    import time

    import torch

    torch.set_num_threads(1)
    for name in (sys.argv[2:] or list(CASES)):
        t0 = time.time()
        CASES[name]()
        print(f"[case {name}: {time.time() - t0:.1f} s]", flush=True)
    print("ALL CASES OK")
