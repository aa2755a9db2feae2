"""Flat PQ scan + rerank tail (csrc/lm_pq_flat_impl.h: k_pq_flat_scan, k_pq_flat_merge; lm_pq_scan, lm_pq_flat_search*) against the reference
composed in tests/pq_flat_ref_util.py: labels equal, distance BITS equal, no tolerance anywhere.  The shapes and inputs live here;
tests/test_gpu_pq_flat_search.py runs them on the MI355X at the full sizes, tests/test_pq_flat_search.py runs them against the host build of the
library (tests/hip_emul/build_emul_lib.py, a thread per lane -- 1024 of them per workgroup -- hence the smaller shapes of `be.emulated`):
    python -m tests.emulated_pq_flat_cases <path/to/libleann_mi355x_emul.so> [case ...]"""
import sys
from pathlib import Path

import numpy as np

from tests import pq_flat_ref_util as fu
from tests.emulated_pq_search_cases import GpuBackend, HostBackend, _load, _uniform_pq, flat_csr  # noqa: F401  (the two worlds and their providers)
from tests.pq_flat_ref_util import IP, L2

CASES = {}
CHUNKS_8 = [3, 0, 7, 1, 9, 8, 12, 10]  # unequal lengths, a zero-length chunk, ends at 50 < 64


def _check(be, tag, cb, codes, q, L, metric, mask=None, off=None, stray=False, **kw):
    words = None if mask is None else fu.bitmap(mask, stray)
    rc, lab, dist, ok = fu.scan(be, cb, codes, q, L, metric, words, off, **kw)
    d = kw.get("d")
    el, ed = fu.expected_scan(cb, codes, q if d is None else q, L, metric, mask, off)
    good = rc == 0 and ok and fu.same(lab, dist, el, ed)
    print(f"pq_scan {tag} n={codes.shape[0]} m={codes.shape[1]} nq={q.shape[0]} L={L} metric={metric} "
          f"plan={fu.plan(codes.shape[0], q.shape[0], codes.shape[1], L)}: {'ok' if good else 'MISMATCH'}", flush=True)
    assert good, (tag, rc, ok)
    return lab, dist


def _queries(nq, d, seed, ld=None):
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((nq, ld or d)).astype(np.float32)
    return q


# ---- slicing ---------------------------------------------------------------------------------------------------------------------
def slicing_grid(emulated: bool):
    """(ntotal, nq kind, L): the issue's grid on the GPU; in the emulation a walk through it that still meets every value of every axis."""
    m = 8
    one = 2048  # the plan's one-slice limit
    assert fu.plan(one, 1, m, 10)[1] == 1 and fu.plan(one + 1, 1, m, 10)[1] == 2 and fu.plan(2 * one + 1, 1, m, 10)[1] == 3 and fu.plan(20000, 1, m, 10)[1:] == (10, 2016)
    ns = (0, 1, 31, 33, one, one + 1, 2 * one + 1, 20000)
    if not emulated:
        return [(n, nqk, L) for n in ns for nqk in (0, 1, 2) for L in (1, 10, 64, 1024)]
    return [(0, 1, 10), (1, 0, 1), (31, 2, 64), (33, 0, 1024), (one, 1, 1), (one + 1, 2, 10), (2 * one + 1, 0, 64), (20000, 0, 10)]


def case_slicing(be, grid=None):
    """m = 8 at d = 64 (eight queries per tile up to L = 112, four at L = 1024), every second shape under a random half allow-list, metrics in
    turn.  nq kind 0 / 1 / 2 = 1, 3, one more than a query tile."""
    m, d = 8, 64
    for i, (n, nqk, L) in enumerate(slicing_grid(be.emulated) if grid is None else grid):
        qt = fu.plan(n, 1, m, L)[0]
        nq = (1, 3, qt + 1)[nqk]
        cb, codes, _ = fu.random_pq(n, d, m, 100 + i)
        mask = (np.random.default_rng(i).random(n) < 0.5) if i % 2 else None
        _check(be, "slicing", cb, codes, _queries(nq, d, 200 + i), L, (L2, IP)[i % 2] if i % 4 < 2 else (IP, L2)[i % 2], mask)


CASES["slicing"] = case_slicing

# ---- layouts ---------------------------------------------------------------------------------------------------------------------
LAYOUTS = [
    # (name, m, d, chunk lengths or None, GPU only)
    ("m4-d8", 4, 8, None, False), ("m8-d64", 8, 64, None, False), ("m96-d384", 96, 384, None, False), ("m48-d384", 48, 384, None, False),
    ("m8-d64-chunked", 8, 64, CHUNKS_8, False),
    ("m16-d64", 16, 64, None, True), ("m32-d64", 32, 64, None, True), ("m64-d128", 64, 128, None, True), ("m128-d256", 128, 256, None, True),  # the other piece counts
    ("m20-d40", 20, 40, None, True),  # dword loop at a width that is no multiple of 16
]


def case_layouts(be, layouts=None):
    """Every table shape and every compiled form of the row fetch, both metrics, queries at a row stride above d, a code array that does not
    start on a 16-byte boundary (the dword form at m = 16)."""
    n = 300 if be.emulated else 2500
    for name, m, d, lens, gpu_only in LAYOUTS:
        if (layouts is not None and name not in layouts) or (be.emulated and gpu_only):
            continue
        cb, codes, off = fu.random_pq(n, d, m, 7 + m, lens)
        qt = fu.plan(n, 1, m, 10)[0]
        assert (name != "m96-d384" or qt == 1) and (name != "m48-d384" or qt > 1)
        nq = min(qt + 1, 3)
        for metric in (IP, L2):
            _check(be, name, cb, codes, _queries(nq, d, 31 + metric), 10, metric, off=off, d=d)
            if m in (8, 48) or not be.emulated:
                qw = _queries(nq, d, 33 + metric, ld=d + 24)
                lab, dist = _check(be, name + "/ldq", cb, codes, qw, 10, metric, off=off, d=d)
                assert fu.same(lab, dist, *fu.expected_scan(cb, codes, np.ascontiguousarray(qw[:, :d]), 10, metric, None, off))  # columns >= d do not count
    if layouts is not None and "m16-d64" not in layouts:
        return
    cb, codes, _ = fu.random_pq(n, 64, 16, 5)
    a = _check(be, "m16 aligned", cb, codes, _queries(2, 64, 6), 10, L2)
    b = _check(be, "m16 at +4 bytes", cb, codes, _queries(2, 64, 6), 10, L2, misalign=4)
    assert fu.same(*a, *b)


CASES["layouts"] = case_layouts


# ---- ranking ---------------------------------------------------------------------------------------------------------------------
def case_ranking(be):
    """Equal code rows on either side of the slice boundaries, a NaN coordinate, the zero query under inner product, L above the row count."""
    m, d, L = 8, 64, 64
    n = 4097  # three slices
    S, rows = fu.plan(n, 2, m, L)[1:]
    assert S == 3
    cb, codes, _ = fu.random_pq(n, d, m, 11)
    codes[rows - 3 : rows + 3] = codes[7]  # one row's code on both sides of the first boundary
    codes[2 * rows - 2 : 2 * rows + 2] = codes[7]
    codes[n - n // 3 :] = codes[: n // 3]  # and a third of the array again, two slices further on
    q = _queries(2, d, 12)
    for metric in (IP, L2):
        lab, dist = _check(be, "ties", cb, codes, q, L, metric)
        tie = (dist[:, :-1] == dist[:, 1:]) & (lab[:, :-1] // rows != lab[:, 1:] // rows)
        assert tie.any() and (lab[:, :-1][tie] < lab[:, 1:][tie]).all()  # equal ADC across slices: the lower id first
    qn = _queries(2, d, 13)
    qn[0, 5] = np.nan
    for metric in (IP, L2):
        lab, dist = _check(be, "nan", cb, codes[:300], qn, 10, metric)
        assert np.array_equal(lab[0], np.arange(10)) and np.isinf(dist[0]).all()  # every key +inf: ids ascending
    lab, dist = _check(be, "zero/ip", cb, codes[:300], np.zeros((1, d), np.float32), 10, IP)
    assert np.array_equal(lab[0], np.arange(10)) and (dist.view(np.uint32) == 0x80000000).all()  # -(+0) = -0.0
    lab, dist = _check(be, "L > rows", cb, codes[:40], q, 64, L2)
    assert (lab[:, 40:] == -1).all() and np.isposinf(dist[:, 40:]).all() and (lab[:, :40] >= 0).all()
    lab, dist = _check(be, "L > rows", cb, codes[:40], q, 64, IP)
    assert (lab[:, 40:] == -1).all() and np.isneginf(dist[:, 40:]).all()


CASES["ranking"] = case_ranking


# ---- allow-list ------------------------------------------------------------------------------------------------------------------
def case_allow_list(be):
    """NULL, nobody, one bit in the last word, about 1 % at random, everybody with garbage above ntotal in the last word: each equals the
    reference on the compacted code array with the ids mapped back."""
    m, d, L = 8, 64, 10
    n = 2093 if be.emulated else 6221  # n % 32 != 0, more than one slice
    cb, codes, _ = fu.random_pq(n, d, m, 21)
    q = _queries(2, d, 22)
    rng = np.random.default_rng(23)
    for metric in (IP, L2):
        full, fd = _check(be, "null", cb, codes, q, L, metric)
        lab, _ = _check(be, "none", cb, codes, q, L, metric, np.zeros(n, bool))
        assert (lab == -1).all()
        one = np.zeros(n, bool)
        one[n - 1] = True
        lab, _ = _check(be, "last bit", cb, codes, q, L, metric, one)
        assert (lab[:, 0] == n - 1).all() and (lab[:, 1:] == -1).all()
        mask = rng.random(n) < 0.01
        lab, dist = _check(be, "1 %", cb, codes, q, L, metric, mask)
        allowed = np.flatnonzero(mask)
        cl, cd = fu.expected_scan(cb, codes[allowed], q, L, metric)  # the compacted array: a monotone id map keeps the tie-break
        assert fu.same(lab, dist, np.where(cl >= 0, allowed[np.clip(cl, 0, None)], -1), cd)
        lab, dist = _check(be, "all + stray", cb, codes, q, L, metric, np.ones(n, bool), stray=True)
        assert fu.same(lab, dist, full, fd)


CASES["allow_list"] = case_allow_list


# ---- argument checking -----------------------------------------------------------------------------------------------------------
def case_argument_checking(be):
    """Everything the header rejects returns LM_EINVAL and touches no buffer; nq == 0 is fine and writes nothing; the workspace size is the plan's."""
    from leann_amd import _lib

    lib = _lib.load()
    m, d = 8, 64
    cb, codes, _ = fu.random_pq(40, d, m, 1)
    q = _queries(2, d, 2)
    off8 = fu.offsets(m, d, CHUNKS_8)
    cbc = np.zeros(256 * int(off8[-1]), np.float32)

    def bad_off(**ch):
        o = off8.copy()
        for i, v in ch.items():
            o[int(i[1:])] = v
        return o

    bad = [dict(m=0), dict(m=-4), dict(m=6), dict(m=4100), dict(d=60), dict(ldq=63), dict(L=0), dict(L=-1), dict(L=fu.MAX_L + 1), dict(metric=2),
           dict(metric=-1), dict(nq=-1), dict(ntotal=-1), dict(ntotal=2**31), dict(ws_short=1), dict(null=("codes",)), dict(null=("cb",)), dict(null=("q",)),
           dict(null=("D",)), dict(null=("L",)), dict(null=("ws",)),
           dict(m=160, L=10),  # a table of 160 KB: the scan state does not fit the LDS
           dict(misalign=2),  # code rows are read as dwords
           dict(cb=cbc, off=bad_off(o0=1)), dict(cb=cbc, off=bad_off(o3=2)), dict(cb=cbc, off=off8, d=49)]
    for over in bad:
        a = dict(L=10, metric=L2)
        a.update(over)
        cbx = a.pop("cb", cb)
        mm = a.get("m")
        cd = codes if mm in (None, 0, -4, 6) or mm < 0 else np.zeros((40, mm), np.uint8)
        if "d" not in a and mm is not None:
            a["d"] = d
        rc, _, _, untouched = fu.scan(be, cbx, cd, q, a.pop("L"), a.pop("metric"), None, a.pop("off", None), **a)
        assert rc == _lib.LM_EINVAL and untouched, (over, rc, untouched)
        try:
            _lib.check(rc, "lm_pq_scan")
        except ValueError:
            pass
        else:
            raise AssertionError("LM_EINVAL must map to ValueError")
    rc, _, _, untouched = fu.scan(be, cb, codes, q, 10, L2, nq=0)
    assert rc == 0 and untouched
    rc, lab, dist, ok = fu.scan(be, cb, codes, q, 10, L2, ntotal=0, null=("codes",))
    assert rc == 0 and ok and (lab == -1).all() and np.isposinf(dist).all()
    assert lib.lm_pq_scan_workspace_bytes(40, 2, 8, 10) == 1 * 2 * 10 * 8 and lib.lm_pq_scan_workspace_bytes(4097, 1, 8, 7) == 3 * 7 * 8
    assert lib.lm_pq_scan_workspace_bytes(40, 2, 160, 10) == 0 and lib.lm_pq_scan_workspace_bytes(40, 2, 8, fu.MAX_L + 1) == 0
    print("argument checking: ok", flush=True)


CASES["argument_checking"] = case_argument_checking


# ---- index form ------------------------------------------------------------------------------------------------------------------
def _index_world(be, metric, n, d=48, m=8, seed=5):
    from leann_amd.index import Mi355xIndex
    from tests.util import clustered

    x = clustered(n, d, seed, n_centers=8, sigma=0.5)
    rng = np.random.default_rng(seed)
    adj = [rng.choice(n, 6, replace=False).astype(np.int32) for _ in range(n)]
    g = flat_csr(adj, d, metric, 0)
    cb, codes = _uniform_pq(x, m, iters=2)
    idx = Mi355xIndex.from_csr(g)
    be.prepare(idx)
    return x, cb, codes, idx


def _stats(idx):
    st = idx.stats()
    return int(st["ndis"]), int(st["nunique"]), int(st["nrounds"]), int(st["nexpand"])


def case_index(be):
    """lm_pq_flat_search on an index: LM_ESTATE without codes and without an embedding source, the provider path (ONE sorted unique request,
    the stats), fp32 and fp16 tables, skip_search_reorder, host and device entry, and -- L >= the allowed rows -- equality with
    lm_index_search_exact under the same allow-list."""
    n = 200 if be.emulated else 700
    for metric in (IP, L2):
        x, cb, codes, idx = _index_world(be, metric, n)
        q = (x[:3] + 0.01).astype(np.float32)
        rng = np.random.default_rng(9)
        mask = rng.random(n) < 0.3
        na = int(mask.sum())
        k, L = 5, 24
        prm = idx.make_pq_params(L, 1, use_deferred_fetch=True)
        try:
            idx.pq_flat_search(q, k, prm, allowed=mask)
        except RuntimeError:  # LM_ESTATE: no codes yet
            pass
        else:
            raise AssertionError("pq_flat_search without codes must raise")
        idx.attach_pq(cb, codes)
        try:
            idx.pq_flat_search(q, k, prm, allowed=mask)
        except RuntimeError:  # LM_ESTATE: deferred fetch with neither a provider nor a table
            pass
        else:
            raise AssertionError("deferred fetch without an embedding source must raise")
        for bad in (dict(complexity=0), dict(complexity=fu.MAX_L + 1)):
            try:
                idx.pq_flat_search(q, k, idx.make_pq_params(bad["complexity"], 1), allowed=mask)
            except ValueError:
                pass
            else:
                raise AssertionError(f"{bad} must raise ValueError")
        # PQ order: no embedding source at all
        got = idx.pq_flat_search(q, k, idx.make_pq_params(L, 7), allowed=mask)
        el, ed, union = fu.expected_search(cb, codes, x, q, k, L, metric, mask, rerank=False)
        assert fu.same(*got, el, ed) and _stats(idx) == (na * 3, 0, 1, 0), ("pq order", _stats(idx))
        # provider
        fn, calls = be.provider(x, int(idx.info.d_padded))
        idx.set_provider(fn)
        got = idx.pq_flat_search(q, k, prm, allowed=mask)
        el, ed, union = fu.expected_search(cb, codes, x, q, k, L, metric, mask)
        assert len(calls) == 1 and np.array_equal(calls[0], union), (len(calls), calls[0][:8], union[:8])
        assert fu.same(*got, el, ed) and _stats(idx) == (na * 3, len(union), 1, 0), ("provider", _stats(idx))
        assert set(got[0].reshape(-1)) <= set(np.flatnonzero(mask))
        got = idx.pq_flat_search(q, k, idx.make_pq_params(L, 1, use_deferred_fetch=True, skip_search_reorder=True), allowed=mask)
        assert len(calls) == 1 and fu.same(*got, *fu.expected_search(cb, codes, x, q, k, L, metric, mask, rerank=False)[:2])
        if not be.emulated:  # the device entry: the same bits
            import torch

            dl, dd = idx.pq_flat_search_device(torch.from_numpy(q).cuda(), k, prm, allowed=mask)
            assert fu.same(dl.cpu().numpy(), dd.cpu().numpy(), el, ed) and len(calls) == 2
            words = torch.from_numpy(fu.bitmap(mask).view(np.int32)).cuda()
            dl, dd = idx.pq_flat_search_device(torch.from_numpy(q).cuda(), k, prm, allowed=words)
            assert fu.same(dl.cpu().numpy(), dd.cpu().numpy(), el, ed)
        # no allow-list, k > complexity: L = k
        got = idx.pq_flat_search(q, 30, prm)
        assert fu.same(*got, *fu.expected_search(cb, codes, x, q, 30, L, metric)[:2])
        idx.set_provider(None)
        # stored tables
        for tab in (x, x.astype(np.float16)):
            idx.attach_table(tab)
            wide = tab.astype(np.float32)
            got = idx.pq_flat_search(q, k, idx.make_pq_params(L, 1), allowed=mask)
            assert fu.same(*got, *fu.expected_search(cb, codes, x, q, k, L, metric, mask, table=wide)[:2]), ("table", tab.dtype)
            got = idx.pq_flat_search(q, k, idx.make_pq_params(L, 1, skip_search_reorder=True), allowed=mask)
            assert fu.same(*got, *fu.expected_search(cb, codes, x, q, k, L, metric, mask, rerank=False)[:2])
            # every allowed row reranked: the exact filtered search, bit for bit
            few = np.zeros(n, bool)
            few[rng.permutation(n)[:50]] = True
            gl, gd = idx.pq_flat_search(q, 10, idx.make_pq_params(64, 1), allowed=few)
            xd, xl = idx.search_exact(q, 10, allowed=few)
            assert fu.same(gl, gd, xl, xd), ("exact cross-check", tab.dtype)
        # the graph search on the same handle is what it was
        before = idx.pq_search(q, k, idx.make_pq_params(L, 2))
        idx.pq_flat_search(q, k, idx.make_pq_params(L, 1), allowed=mask)
        after = idx.pq_search(q, k, idx.make_pq_params(L, 2))
        assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
        idx.close()
        print(f"index form metric={metric}: ok", flush=True)


CASES["index"] = case_index


# ---- lm_pq_batch_search before and after the rerank tail was shared ---------------------------------------------------------------
def batch_search_fixture(be):
    """The fixed small index of the off-by-default check -> (labels, distance bits, stats) of lm_pq_batch_search through the provider and the table."""
    x, _, _, idx = _index_world(be, L2, 200, seed=17)
    rng = np.random.default_rng(18)  # numpy only: the same quantiser on every machine
    cb, codes = rng.standard_normal((8, 256, 6)).astype(np.float32), rng.integers(0, 256, (200, 8), dtype=np.uint8)
    idx.attach_pq(cb, codes)
    q = (x[:4] + 0.02).astype(np.float32)
    out = []
    fn, calls = be.provider(x, int(idx.info.d_padded))
    idx.set_provider(fn)
    lab, dist = idx.pq_search(q, 5, idx.make_pq_params(16, 2, use_deferred_fetch=True))
    st = idx.stats()
    out.append((lab.tolist(), dist.view(np.uint32).tolist(), [int(st[f]) for f in ("ndis", "nexpand", "nrounds", "nunique")]))
    idx.set_provider(None)
    idx.attach_table(x)
    lab, dist = idx.pq_search(q, 5, idx.make_pq_params(16, 2))
    st = idx.stats()
    out.append((lab.tolist(), dist.view(np.uint32).tolist(), [int(st[f]) for f in ("ndis", "nexpand", "nrounds", "nunique")]))
    idx.close()
    return out


# ---- the index form's rejections ----------------------------------------------------------------------------------------------------
def _raw_flat_search(be, idx, device_form, n, q, k, prm, words=None, null=()):
    """lm_pq_flat_search (host pointers) or lm_pq_flat_search_device (the world's device pointers) called directly on sentinel-filled label and
    distance buffers -> (rc, untouched): untouched says that every element of both buffers still holds its fill."""
    import ctypes as C

    from tests.gpu_abi_util import FILL_I64

    M = fu.mem(be) if device_form else fu._HostMem()
    own = max(n, 1) * max(k, 1) + 64
    hq, pq = M.put(np.ascontiguousarray(q, np.float32))
    hw, pw = (None, None) if words is None else M.put(words)
    D, pD = M.full(own, np.nan, np.float32)
    Lb, pL = M.full(own, FILL_I64, np.int64)
    ptr = dict(x=pq, L=pL, D=pD, params=None if prm is None else C.byref(prm), idx=idx._h)
    for name in null:
        ptr[name] = None
    fn = idx._lib.lm_pq_flat_search_device if device_form else idx._lib.lm_pq_flat_search
    rc = fn(ptr["idx"], n, ptr["x"], k, ptr["params"], pw, ptr["L"], ptr["D"])
    hD, hL = M.get(D), M.get(Lb)
    return rc, bool(np.isnan(hD).all() and (hL == FILL_I64).all())


def case_index_rejections(be):
    """Every LM_EINVAL / LM_ESTATE case of lm_pq_flat_search and lm_pq_flat_search_device, each on pre-filled outputs that must keep their fill:
    no codes; deferred fetch with neither a provider nor a table; recompute_neighbors != 0; complexity < 1; max(complexity, k) above
    LM_PQ_FLAT_MAX_L; k < 1; n < 0; NULL index / params / buffers; a scan state that does not fit the LDS (m = 144, L = 300)."""
    from leann_amd import _lib
    from leann_amd.index import Mi355xIndex

    n = 120
    x, cb, codes, idx = _index_world(be, L2, n)
    q = (x[:2] + 0.01).astype(np.float32)
    words = fu.bitmap(np.random.default_rng(2).random(n) < 0.5)
    mk = idx.make_pq_params

    def rn():
        p = mk(16, 1)
        p.recompute_neighbors = 1
        return p

    def both(tag, want, k, prm, nq=2, null=(), index=idx):
        for device_form in (False, True):
            rc, untouched = _raw_flat_search(be, index, device_form, nq, q, k, prm, words, null)
            assert rc == want and untouched, (tag, device_form, rc, untouched)

    both("no codes", _lib.LM_ESTATE, 5, mk(16, 1))
    idx.attach_pq(cb, codes)
    both("deferred fetch, no source", _lib.LM_ESTATE, 5, mk(16, 1, use_deferred_fetch=True))
    both("recompute_neighbors", _lib.LM_EINVAL, 5, rn())
    both("complexity 0", _lib.LM_EINVAL, 5, mk(0, 1))
    both("complexity -3", _lib.LM_EINVAL, 5, mk(-3, 1))
    both("complexity above the limit", _lib.LM_EINVAL, 5, mk(fu.MAX_L + 1, 1))
    both("k above the limit", _lib.LM_EINVAL, fu.MAX_L + 1, mk(16, 1))
    both("k 0", _lib.LM_EINVAL, 0, mk(16, 1))
    both("n < 0", _lib.LM_EINVAL, 5, mk(16, 1), nq=-1)
    both("NULL params", _lib.LM_EINVAL, 5, None)
    both("NULL index", _lib.LM_EINVAL, 5, mk(16, 1), null=("idx",))
    for name in ("x", "L", "D"):
        both("NULL " + name, _lib.LM_EINVAL, 5, mk(16, 1), null=(name,))
    for prm, exc in ((rn(), ValueError), (mk(0, 1), ValueError)):  # and what the wrapper raises
        try:
            idx.pq_flat_search(q, 5, prm, allowed=None)
        except exc:
            pass
        else:
            raise AssertionError("must raise")
    rc, untouched = _raw_flat_search(be, idx, False, 2, q, 5, mk(16, 1), words)  # the same call, accepted: the buffers are written
    assert rc == 0 and not untouched
    idx.close()
    # a table of 144 KB leaves room for lists of 256 keys: L = 300 is refused before anything is staged or launched, L = 256 runs
    d = m = 144
    rng = np.random.default_rng(3)
    xw = rng.standard_normal((40, d)).astype(np.float32)
    wide = Mi355xIndex.from_csr(flat_csr([np.array([(i + 1) % 40], np.int32) for i in range(40)], d, L2, 0))
    be.prepare(wide)
    cbw, cdw, _ = fu.random_pq(40, d, m, 4)
    wide.attach_pq(cbw, cdw)
    assert fu.plan(40, 2, m, 300)[0] == 0 and fu.plan(40, 2, m, 256)[0] == 1
    qw = xw[:2].copy()
    for device_form in (False, True):
        rc, untouched = _raw_flat_search(be, wide, device_form, 2, qw, 5, wide.make_pq_params(300, 1))
        assert rc == _lib.LM_EINVAL and untouched, ("LDS", device_form, rc, untouched)
    got = wide.pq_flat_search(qw, 5, wide.make_pq_params(256, 1))
    assert fu.same(*got, *fu.expected_search(cbw, cdw, xw, qw, 5, 256, L2, rerank=False)[:2])
    wide.close()
    print("index form rejections: ok", flush=True)


CASES["index_rejections"] = case_index_rejections


# lm_pq_batch_search on that index at the parent commit (before the tail became a function of its own): per mode (provider, table) the labels, the
# distance bits and (ndis, nexpand, nrounds, nunique)
BATCH_SEARCH_AT_PARENT = [
    ([[125, 153, 191, 81, 58], [12, 191, 143, 133, 81], [98, 77, 153, 81, 141], [133, 141, 70, 12, 35]],
     [[1055235394, 1057995468, 1072062376, 1072248053, 1072292154], [1049795969, 1052114532, 1052754774, 1069216309, 1069753059],
      [1051607520, 1053629860, 1070332958, 1071114323, 1072002080], [1042243705, 1050491369, 1051882132, 1068757812, 1069355586]], [343, 76, 13, 23]),
    ([[125, 153, 191, 81, 58], [12, 191, 143, 133, 81], [98, 77, 153, 81, 141], [133, 141, 70, 12, 35]],
     [[1055235394, 1057995468, 1072062376, 1072248053, 1072292154], [1049795969, 1052114532, 1052754774, 1069216309, 1069753059],
      [1051607520, 1053629860, 1070332958, 1071114323, 1072002080], [1042243705, 1050491369, 1051882132, 1068757812, 1069355586]], [343, 76, 13, 0]),
]


def case_batch_search_unchanged(be):
    """The traversal path after its rerank tail was moved into pq_rerank_tail: the recorded labels, distance bits and stats."""
    got = batch_search_fixture(be)
    assert [tuple(g) for g in got] == [tuple(e) for e in BATCH_SEARCH_AT_PARENT], got
    print("lm_pq_batch_search as at the parent commit: ok", flush=True)


CASES["batch_search_unchanged"] = case_batch_search_unchanged


# ---- the two searchers -----------------------------------------------------------------------------------------------------------
def case_wiring(be):
    """pq.pq_scan_kernel and the searchers' keywords that need no encoder: pq_flat on a table-carrying bundle (recompute_embeddings=False),
    refused without a quantiser (the message names pq_bytes), refused on a pruned bundle with recompute_embeddings=False, allowed_ids alone
    still a ValueError, the DiskANN-style searcher's two keywords."""
    import tempfile

    import torch

    from leann_amd._compat import BACKEND_REGISTRY
    from leann_amd.backend import write_leann_bundle
    from leann_amd.pq import pq_scan_kernel
    from tests.util import clustered

    n, d = (300, 48) if be.emulated else (900, 48)
    x = clustered(n, d, 5, n_centers=8, sigma=0.5)
    q = (x[:3] + 0.01).astype(np.float32)
    mask = np.random.default_rng(4).random(n) < 0.2
    cb, codes = _uniform_pq(x, 8, iters=2)
    dev = "cpu" if be.emulated else "cuda"
    for metric, name in ((IP, "mips"), (L2, "l2")):
        dd, ll = pq_scan_kernel(torch.from_numpy(codes).to(dev), torch.from_numpy(cb).to(dev), torch.from_numpy(q).to(dev), 12, name, allowed=mask)
        assert tuple(dd.shape) == (3, 12) and dd.dtype == torch.float32 and ll.dtype == torch.int64
        assert fu.same(ll.cpu().numpy(), dd.cpu().numpy(), *fu.expected_scan(cb, codes, q, 12, metric, mask))
    print("pq_scan_kernel: ok", flush=True)
    texts = [f"passage {i}" for i in range(n)]
    model = "sentence-transformers/all-MiniLM-L6-v2"
    ids = [int(v) for v in np.flatnonzero(mask)]
    with tempfile.TemporaryDirectory() as td:
        p = str(Path(td) / "full.leann")
        write_leann_bundle(p, texts, x, model, distance_metric="l2", M=6, efConstruction=30, is_recompute=False, pq_bytes=8)
        s = BACKEND_REGISTRY["mi355x"].searcher(p)
        idx = s._ensure_index_loaded()
        z = np.load(Path(td) / "full_pq.npz")
        r = s.search(q, 6, recompute_embeddings=False, complexity=20, pq_flat=True, allowed_ids=ids)
        el, ed, _ = fu.expected_search(z["codebooks"], z["codes"], x, q, 6, 20, L2, mask)
        assert r["labels"] == [[str(int(v)) for v in row] for row in el] and fu.same(el, r["distances"], el, ed)
        r2 = s.search(q, 6, recompute_embeddings=False, complexity=20, pq_flat=True, allowed_ids=mask)
        assert r2["labels"] == r["labels"]
        for kw, exc in ((dict(recompute_embeddings=False, allowed_ids=[1]), ValueError), (dict(recompute_embeddings=False, exact=True, pq_flat=True), ValueError)):
            try:
                s.search(q, 6, **kw)
            except exc:
                pass
            else:
                raise AssertionError(f"{kw} must raise {exc.__name__}")
        del idx
        s.cleanup()
        p1 = str(Path(td) / "nopq.leann")
        write_leann_bundle(p1, texts, x, model, distance_metric="l2", M=6, efConstruction=30, is_recompute=False)
        s = BACKEND_REGISTRY["mi355x"].searcher(p1)
        try:
            s.search(q, 6, recompute_embeddings=False, pq_flat=True, allowed_ids=ids)
        except RuntimeError as ex:
            assert "pq_bytes" in str(ex)
        else:
            raise AssertionError("pq_flat without a quantiser must raise")
        s.cleanup()
        p2 = str(Path(td) / "pruned.leann")
        write_leann_bundle(p2, texts, x, model, distance_metric="l2", M=6, efConstruction=30, pq_bytes=8)
        s = BACKEND_REGISTRY["mi355x"].searcher(p2)
        try:
            s.search(q, 6, recompute_embeddings=False, pq_flat=True, allowed_ids=ids)
        except RuntimeError as ex:
            assert "Recompute is required" in str(ex)
        else:
            raise AssertionError("pq_flat with recompute_embeddings=False on a pruned index must raise")
        s.cleanup()
        p3 = str(Path(td) / "dk.leann")
        write_leann_bundle(p3, texts, x, model, backend_name="mi355x_diskann", distance_metric="l2")
        s = BACKEND_REGISTRY["mi355x_diskann"].searcher(p3)
        try:
            s.search(q, 6, allowed_ids=[1])
        except ValueError:
            pass
        else:
            raise AssertionError("allowed_ids without pq_flat must raise")
        z = np.load(Path(td) / "dk_pq.npz")  # the bundle keeps its vectors: the rerank reads the stored table
        r = s.search(q, 6, complexity=20, pq_flat=True, allowed_ids=ids)
        el, ed, _ = fu.expected_search(z["codebooks"], z["codes"], x, q, 6, 20, L2, mask)
        assert r["labels"] == [[str(int(v)) for v in row] for row in el] and fu.same(el, r["distances"], el, ed)
        s.cleanup()
    print("backend wiring: ok", flush=True)


CASES["wiring"] = case_wiring


if __name__ == "__main__":
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    _load(sys.argv[1])
    import time

    import torch

    torch.set_num_threads(1)
    be = HostBackend()
    for name in (sys.argv[2:] or list(CASES)):
        t0 = time.time()
        CASES[name](be)
        print(f"[case {name}: {time.time() - t0:.1f} s]", flush=True)
    print("ALL CASES OK")
