"""lm_index_search_filtered (csrc/lm_filter_impl.h: k_filter_collect) against the reference composed in tests/filtered_ref_util.py: labels equal,
distance BITS equal, (ndis, nexpand, nrounds, nunique) and the provider's per-round request lists equal to the unfiltered call's,
"filtered_allowed_evals" equal to the reference's sum of |E n allowed| -- no tolerance anywhere.  The shapes and inputs live here;
tests/test_gpu_filtered_search.py runs them on the MI355X, tests/test_filtered_search.py against the host build of the library
(tests/hip_emul/build_emul_lib.py, a thread per lane):
    python -m tests.emulated_filtered_cases <path/to/libleann_mi355x_emul.so> [case ...]"""
import ctypes as C
import sys
from pathlib import Path

import numpy as np

from tests import filtered_ref_util as fr
from tests import pq_flat_ref_util as fu
from tests.emulated_pq_search_cases import GpuBackend, HostBackend, _load  # noqa: F401  (the two worlds and their providers)
from tests.filtered_ref_util import IP, L2

CASES = {}
N, M = 2000, 8
_WORLDS = {}


class World:
    """A graph of n nodes (M = 8), its table and the reference on it."""

    def __init__(self, n, d, metric, seed, table=None, graph=None, f16=False):
        from leann_amd.hnsw_builder import build_hnsw
        from tests.util import clustered

        self.x = clustered(n, d, seed) if table is None else table
        self.g = build_hnsw(self.x, metric, M=M, ef_construction=40) if graph is None else graph
        self.served = self.x.astype(np.float16) if f16 else self.x  # what a table attach uploads
        self.R = fr.Reference(self.g, self.served.astype(np.float32))
        self.n, self.d, self.metric = n, d, int(self.g.metric_type)

    def queries(self, nq, seed=77):
        from tests.util import queries_near

        return queries_near(self.x, nq, seed)


def world(name):
    """"ip64": 2000 nodes, D = 64, inner product; "l2_100": 2001 nodes (the last allow word has unused bits), D = 100 (padded to 128), L2"""
    if name not in _WORLDS:
        _WORLDS[name] = World(N, 64, "mips", 5) if name == "ip64" else World(N + 1, 100, "l2", 9)
    return _WORLDS[name]


def open_index(be, W, source="provider"):
    """-> (index, the provider's call log or None).  source: "provider", "hub" (provider + a 10 % hub cache), "f32" / "f16" (attached table)"""
    from leann_amd.backend import hub_nodes
    from leann_amd.index import Mi355xIndex

    idx = Mi355xIndex.from_csr(W.g)
    be.prepare(idx)
    if source in ("f32", "f16"):
        idx.attach_table(W.x.astype(np.float16) if source == "f16" else W.x)
        return idx, None
    fn, calls = be.provider(W.R.table, idx.info.d_padded)
    idx.set_provider(fn)
    if source == "hub":
        hubs = np.ascontiguousarray(hub_nodes(W.g, 0.1), np.int32)
        emb = np.ascontiguousarray(fr.pad64(W.R.table)[hubs])
        if be.emulated:
            from leann_amd import _lib

            _lib.check(idx._lib.lm_index_set_hub_cache(idx._h, hubs.ctypes.data_as(C.c_void_p), len(hubs), emb.ctypes.data_as(C.c_void_p)), "hub")
        else:
            import torch

            idx.set_hub_cache(hubs, torch.from_numpy(emb).cuda())
    return idx, calls


def raw(be, idx, device_form, q, k, prm, words=None, n=None, null=()):
    """lm_index_search_filtered (host pointers) or _device (the world's device pointers) on sentinel-filled outputs ->
    (rc, labels [n, k], distances [n, k], untouched: every element of both buffers still holds its fill)"""
    from tests.gpu_abi_util import FILL_I64

    Mm = fu.mem(be) if device_form else fu._HostMem()
    nq = q.shape[0] if n is None else n
    own = max(nq, 0) * max(k, 0)
    hq, pq = Mm.put(np.ascontiguousarray(q, np.float32))
    hw, pw = (None, None) if words is None else Mm.put(words)
    D, pD = Mm.full(own + 64, np.nan, np.float32)
    Lb, pL = Mm.full(own + 64, FILL_I64, np.int64)
    ptr = dict(x=pq, L=pL, D=pD, params=None if prm is None else C.byref(prm), idx=idx._h)
    for name in null:
        ptr[name] = None
    fn = idx._lib.lm_index_search_filtered_device if device_form else idx._lib.lm_index_search_filtered
    rc = fn(ptr["idx"], nq, ptr["x"], k, pw, ptr["D"], ptr["L"], ptr["params"])
    hD, hL = Mm.get(D), Mm.get(Lb)
    untouched = bool(np.isnan(hD).all() and (hL == FILL_I64).all())
    tail = bool(np.isnan(hD[own:]).all() and (hL[own:] == FILL_I64).all())
    assert tail, "wrote past the n x k outputs"
    return rc, hL[:own].reshape(max(nq, 0), max(k, 0)).copy(), hD[:own].reshape(max(nq, 0), max(k, 0)).copy(), untouched


def _stats(idx):
    st = idx.stats()
    return tuple(int(st[f]) for f in ("ndis", "nexpand", "nrounds", "nunique"))


def check(be, tag, W, idx, calls, q, k, mask, ef, beam=1, bs=0, recompute=True, memo=True, max_batch=0, stray=False, device_form=False):
    """One unfiltered and one filtered call with the same params: the filtered result is the reference's, the unfiltered one the oracle's, stats
    and request lists agree between the two (invariant 2), NULL / all ones give lm_index_search's bits (invariant 1).
    -> (expected labels, expected distances, hits per query)"""
    prm = idx.make_params(ef=ef, beam=beam, recompute=recompute, batch_size=bs, recompute_memo=memo, max_batch=max_batch)
    log = calls if calls is not None else []
    log.clear()
    du, lu = idx.search(q, k, prm)
    su, ru = _stats(idx), [c.copy() for c in log]
    log.clear()
    words = None if mask is None else fr.bitmap(mask, stray)
    rc, lf, df, _ = raw(be, idx, device_form, q, k, prm, words)
    sf, rf, ev = _stats(idx), [c.copy() for c in log], idx.get_option("filtered_allowed_evals")
    el, ed, eev, hits = W.R.expected(q, k, mask, ef, beam, bs)
    ul, ud, _, _ = W.R.expected(q, k, None, ef, beam, bs)
    good = rc == 0 and fr.same(lf, df, el, ed) and fr.same(lu, du, ul, ud) and ev == eev and su == sf
    good = good and len(ru) == len(rf) and all(np.array_equal(a, b) for a, b in zip(ru, rf)) and (calls is None or len(rf) > 0)
    if mask is None or mask.all():
        good = good and fr.same(lf, df, lu, du)
    print(f"filtered {tag} n={W.n} d={W.d} metric={W.metric} nq={q.shape[0]} k={k} ef={ef} beam={beam} bs={bs}: {'ok' if good else 'MISMATCH'}", flush=True)
    assert good, (tag, rc, ev, eev, su, sf, len(ru), len(rf))
    return el, ed, hits


def half(W, seed=1):
    return np.random.default_rng(seed).random(W.n) < 0.5


# ---- sources ---------------------------------------------------------------------------------------------------------------------
def case_sources(be, names=("ip64", "l2_100")):
    """Provider with B = 1 (no memo), B = 3 and B = 70 (memo), memo switched off, a hub cache, fp32 and fp16 tables with "persistent_table" at
    its default (a filtered stored-table search must route to the lock-step rounds)."""
    for name in names:
        W = world(name)
        q = W.queries(70)
        mask = half(W)
        idx, calls = open_index(be, W)
        check(be, "provider B=1", W, idx, calls, q[:1], 10, mask, 64)
        check(be, "provider B=3 memo", W, idx, calls, q[:3], 10, mask, 64, beam=4)
        check(be, "provider B=70 memo", W, idx, calls, q, 10, mask, 16, stray=True)
        check(be, "provider B=3 memo off", W, idx, calls, q[:3], 10, mask, 16, bs=32, memo=False)
        idx.close()
        idx, calls = open_index(be, W, "hub")
        check(be, "provider + hub cache", W, idx, calls, q[:3], 10, mask, 64)
        check(be, "provider + hub cache, memo off", W, idx, calls, q[:3], 10, mask, 16, memo=False)
        idx.close()
        for src in ("f32", "f16"):
            Wt = W if src == "f32" else _f16_world(name)
            idx, _ = open_index(be, Wt, src)
            # ("persistent_table" stays at its default, 1: the unfiltered call of check() runs the persistent kernel, the filtered one must not)
            check(be, f"table {src} B=3", Wt, idx, None, q[:3], 10, mask, 64, recompute=False)
            check(be, f"table {src} B=70", Wt, idx, None, q, 10, mask, 16, beam=4, recompute=False)
            idx.close()


def _f16_world(name):
    if name + "_f16" not in _WORLDS:
        W = world(name)
        _WORLDS[name + "_f16"] = World(W.n, W.d, None, 0, table=W.x, graph=W.g, f16=True)
    return _WORLDS[name + "_f16"]


CASES["sources"] = case_sources


# ---- parameters ------------------------------------------------------------------------------------------------------------------
def parameter_grid(emulated: bool):
    """(efSearch, k, beam, batch_size) from {16, 64} x {1, 10, 64} x {1, 4} x {0, 32}: the whole product on the GPU; in the emulation a walk
    through it that meets every value of every axis, k = 64 at efSearch 16 and k = 1 with beam 4 and batch_size 32 among them."""
    if not emulated:
        return [(ef, k, beam, bs) for ef in (16, 64) for k in (1, 10, 64) for beam in (1, 4) for bs in (0, 32)]
    return [(16, 64, 1, 0), (16, 1, 4, 32), (64, 10, 4, 0), (64, 64, 1, 32), (16, 10, 1, 32), (64, 1, 1, 0)]


def case_parameters(be, grid=None, name="ip64"):
    """k > efSearch (the pool holds k keys, the stop rule counts against efSearch) and a round with more allowed keys than k among them."""
    W = world(name)
    q = W.queries(3, 78)
    idx, calls = open_index(be, W)
    mask = half(W, 2)
    first = W.R._l0[W.R.seed(q[0])][0]  # query 0's first new-list: the seed's neighbours, all allowed -- a round with more allowed keys than k = 1
    mask[first] = True
    assert len(first) > 1
    for ef, k, beam, bs in parameter_grid(be.emulated) if grid is None else grid:
        check(be, "parameters", W, idx, calls, q, k, mask, ef, beam=beam, bs=bs)
    idx.close()


CASES["parameters"] = case_parameters


# ---- allow-lists -----------------------------------------------------------------------------------------------------------------
DRAW_SEED = {"ip64": 1, "l2_100": 1}  # seeds of the 50 % / 2 % draws: k hits for every query at 50 %, fewer than k for at least one at 2 % (asserted)


def case_allow_lists(be, names=("ip64", "l2_100")):
    """NULL, all ones (with the unused bits of the last word set), all zeros, 50 %, 2 %, one id inside E and one outside, only the seed, only
    the nodes that exist on upper levels (the entry point is allowed and comes back only if it is in E)."""
    for name in names:
        W = world(name)
        q = W.queries(8, 79)
        k, ef = 10, 64
        idx, calls = open_index(be, W)
        check(be, "allow NULL", W, idx, calls, q, k, None, ef)
        check(be, "allow all ones", W, idx, calls, q, k, np.ones(W.n, bool), ef, stray=True)
        el, _, hits = check(be, "allow all zeros", W, idx, calls, q, k, np.zeros(W.n, bool), ef, stray=True)
        assert (el == -1).all() and (hits == 0).all()
        rng = np.random.default_rng(DRAW_SEED[name])
        m50, m2 = rng.random(W.n) < 0.5, rng.random(W.n) < 0.02
        _, _, hits = check(be, "allow 50 %", W, idx, calls, q, k, m50, ef, stray=True)
        assert (hits == k).all(), hits
        _, _, hits = check(be, "allow 2 %", W, idx, calls, q, k, m2, ef, stray=True)
        assert (hits < k).any(), hits
        E = [W.R.evaluated(q[i], k, ef) for i in range(q.shape[0])]
        s0 = W.R.seed(q[0])
        inside = int(E[0][E[0] != s0][0])
        outside = int(np.setdiff1d(np.arange(W.n), np.concatenate(E))[0])
        for tag, ids, want0 in (("one id in E", [inside], 1), ("one id outside E", [outside], 0), ("only the seed", [s0], 1)):
            m = np.zeros(W.n, bool)
            m[ids] = True
            el, _, hits = check(be, "allow " + tag, W, idx, calls, q, k, m, ef)
            assert hits[0] == want0 and (want0 == 0 or el[0, 0] == ids[0]) and (tag != "one id outside E" or (el == -1).all())
        upper = np.asarray(W.g.levels) > 1
        assert upper[W.g.entry_point] and 0 < upper.sum() < W.n
        el, _, _ = check(be, "allow upper-level nodes only", W, idx, calls, q, k, upper, ef)
        assert all((W.g.entry_point in el[i]) <= (W.g.entry_point in E[i]) for i in range(q.shape[0]))
        idx.close()


CASES["allow_lists"] = case_allow_lists


# ---- ranking ---------------------------------------------------------------------------------------------------------------------
def case_ranking(be):
    """Duplicate rows (ties go to the lower id, whichever round brought it), a NaN row among the allowed (ranks as +inf), the zero query under
    ip (-0.0 comes back), a query whose seed has no level-0 neighbours."""
    from tests.util import clustered

    # duplicates: the second half of the table repeats the first
    x = clustered(N, 64, 21)
    x[N // 2 :] = x[: N // 2]
    for metric in ("mips", "l2"):
        W = World(N, 64, metric, 0, table=x)
        q = W.queries(3, 80)
        idx, calls = open_index(be, W)
        el, ed, _ = check(be, "ranking: duplicate rows", W, idx, calls, q, 64, half(W, 3), 64, beam=4)
        tie = (ed[:, :-1] == ed[:, 1:]) & (el[:, 1:] >= 0)
        assert tie.any() and (el[:, :-1][tie] < el[:, 1:][tie]).all()  # premise: ties in the expected lists, lower id first
        idx.close()
    # a NaN row: a level-0-only node that query 0 evaluates (never met by the descent; the walk up to its evaluation does not depend on its row)
    for name in ("ip64", "l2_100"):
        W0 = world(name)
        q = W0.queries(3, 81)
        s = W0.R.seed(q[0])
        r = int([v for v in W0.R.evaluated(q[0], 64, 64) if W0.g.levels[v] == 1 and v != s][0])
        xt = W0.x.copy()
        xt[r, 3] = np.nan
        W = World(W0.n, W0.d, None, 0, table=xt, graph=W0.g)
        assert W.R.seed(q[0]) == s
        E0 = W.R.evaluated(q[0], 64, 64)
        m = np.zeros(W.n, bool)
        m[E0[:20]] = True
        m[r] = True
        assert r in E0
        idx, calls = open_index(be, W)
        el, ed, hits = check(be, "ranking: a NaN row among the allowed", W, idx, calls, q, 64, m, 64)
        assert hits[0] < 64 and el[0, hits[0] - 1] == r and np.isinf(ed[0, hits[0] - 1])
        idx.close()
        idx, _ = open_index(be, W, "f32")
        check(be, "ranking: a NaN row, stored table", W, idx, None, q, 64, m, 64, recompute=False)
        idx.close()
    # the zero query under ip: every distance is -0 -> key +0 -> -0.0 comes back, ids ascending
    W = world("ip64")
    qz = np.zeros((2, W.d), np.float32)
    qz[1] = W.queries(1, 82)[0]
    idx, calls = open_index(be, W)
    el, ed, hits = check(be, "ranking: the zero query under ip", W, idx, calls, qz, 10, half(W, 4), 64)
    assert hits[0] == 10 and (ed[0].view(np.uint32) == 0x80000000).all() and (np.diff(el[0]) > 0).all()
    idx.close()
    # a seed without level-0 neighbours: E is the seed alone
    for name in ("ip64", "l2_100"):
        W0 = world(name)
        q = W0.queries(2, 83)
        s = W0.R.seed(q[0])
        lists = [[ls[0][:0] if i == s else ls[0]] + list(ls[1:]) for i, ls in enumerate(W0.R._l0)]
        W = World(W0.n, W0.d, None, 0, table=W0.x, graph=fr._csr(W0.g, lists, W0.g.entry_point, W0.g.max_level))
        assert W.R.seed(q[0]) == s and W.R.evaluated(q[0], 10, 16).tolist() == [s]
        idx, calls = open_index(be, W)
        for allowed_seed in (True, False):
            m = half(W, 5)
            m[s] = allowed_seed
            el, _, hits = check(be, f"ranking: a seed without neighbours, allowed={allowed_seed}", W, idx, calls, q, 10, m, 16, bs=32)
            assert hits[0] == int(allowed_seed) and el[0, 0] == (s if allowed_seed else -1)
        idx.close()


CASES["ranking"] = case_ranking


# ---- invariants ------------------------------------------------------------------------------------------------------------------
def case_invariants(be, name="l2_100"):
    """Invariant 3 (70 queries at max_batch 0, 32 and 1, each of a few queries alone), host and device entry, two calls in a row with different
    allow-lists, lm_index_search before and after."""
    W = world(name)
    q = W.queries(70, 84)
    k, ef = 10, 16
    m1, m2 = half(W, 6), np.random.default_rng(7).random(W.n) < 0.1
    for src in ("provider", "f32"):
        idx, calls = open_index(be, W, src)
        rec = src == "provider"
        prm = idx.make_params(ef=ef, beam=4, recompute=rec)
        before = idx.search(q, k, prm)
        el, ed, _ = check(be, f"invariants {src}: max_batch 0", W, idx, calls, q, k, m1, ef, beam=4, recompute=rec, stray=True)
        for mb in (32, 1):
            check(be, f"invariants {src}: max_batch {mb}", W, idx, calls, q, k, m1, ef, beam=4, recompute=rec, max_batch=mb, stray=True)
        for i in (0, 33, 69):  # alone: its row of the batch
            rc, l1, d1, _ = raw(be, idx, False, q[i : i + 1], k, prm, fr.bitmap(m1))
            assert rc == 0 and fr.same(l1, d1, el[i : i + 1], ed[i : i + 1]), i
        check(be, f"invariants {src}: device entry", W, idx, calls, q, k, m1, ef, beam=4, recompute=rec, device_form=True, stray=True)
        # no state leaks from one call into the next: a sparser list, none, the first one again -- through both entries
        for dev in (False, True):
            for m in (m2, None, m1, np.zeros(W.n, bool), m1):
                check(be, f"invariants {src}: calls in a row, device={dev}", W, idx, calls, q[:5], k, m, ef, beam=4, recompute=rec, device_form=dev)
        after = idx.search(q, k, prm)
        assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
        idx.close()
    print("invariants: ok", flush=True)


CASES["invariants"] = case_invariants


# ---- rejections ------------------------------------------------------------------------------------------------------------------
def case_rejections(be):
    """Every LM_EINVAL / LM_ESTATE case of both entry points on sentinel-filled outputs that must keep their fill; n == 0; the empty index."""
    from leann_amd import _lib
    from leann_amd.hnsw_builder import build_hnsw
    from leann_amd.index import Mi355xIndex

    W = world("ip64")
    q = W.queries(2, 85)
    words = fr.bitmap(half(W, 8))
    bare = Mi355xIndex.from_csr(W.g)  # neither a provider nor a table
    be.prepare(bare)
    idx, _ = open_index(be, W)
    mk = idx.make_params

    def both(tag, want, k, prm, index=idx, n=None, null=()):
        for device_form in (False, True):
            rc, _, _, untouched = raw(be, index, device_form, q, k, prm, words, n=n, null=null)
            assert rc == want and untouched, (tag, device_form, rc, untouched)

    both("pq_pruning_ratio > 0", _lib.LM_EINVAL, 5, mk(ef=16, prune_ratio=0.5))
    both("k 0", _lib.LM_EINVAL, 0, mk(ef=16))
    both("k -1", _lib.LM_EINVAL, -1, mk(ef=16))
    both("efSearch 0", _lib.LM_EINVAL, 5, mk(ef=0))
    both("efSearch -4", _lib.LM_EINVAL, 5, mk(ef=-4))
    both("batch_size -1", _lib.LM_EINVAL, 5, mk(ef=16, batch_size=-1))
    both("NULL params", _lib.LM_EINVAL, 5, None)
    both("NULL index", _lib.LM_EINVAL, 5, mk(ef=16), null=("idx",))
    both("n < 0", _lib.LM_EINVAL, 5, mk(ef=16), n=-1)
    for name in ("x", "L", "D"):
        both("NULL " + name, _lib.LM_EINVAL, 5, mk(ef=16), null=(name,))
    both("no provider", _lib.LM_ESTATE, 5, mk(ef=16, recompute=True), index=bare)
    both("no table", _lib.LM_ESTATE, 5, mk(ef=16, recompute=False), index=bare)
    both("no table (a provider is not one)", _lib.LM_ESTATE, 5, mk(ef=16, recompute=False))
    both("n == 0", 0, 5, mk(ef=16), n=0)
    both("n == 0 on an index without a source", 0, 5, mk(ef=16), index=bare, n=0)
    for device_form in (False, True):  # the same call, accepted: the buffers are written
        rc, _, _, untouched = raw(be, idx, device_form, q, 5, mk(ef=16), words)
        assert rc == 0 and not untouched
    try:
        idx.search_filtered(q, 5, mk(ef=16, prune_ratio=0.5), allowed=[1, 2])
    except ValueError:
        pass
    else:
        raise AssertionError("must raise")
    bare.close()
    idx.close()
    # the empty index: every slot gets the empty values, whatever is attached
    for metric, inf in (("l2", np.inf), ("mips", -np.inf)):
        empty = Mi355xIndex.from_csr(build_hnsw(np.zeros((0, 64), np.float32), metric))
        be.prepare(empty)
        for device_form in (False, True):
            rc, lab, dist, _ = raw(be, empty, device_form, np.zeros((3, 64), np.float32), 4, mk(ef=16), None)
            assert rc == 0 and (lab == -1).all() and (dist == inf).all(), (metric, device_form)
        assert empty.get_option("filtered_allowed_evals") == 0
        empty.close()
    print("rejections: ok", flush=True)


CASES["rejections"] = case_rejections


# ---- wiring ----------------------------------------------------------------------------------------------------------------------
def case_wiring(be):
    """Mi355xIndex.search_filtered / search_filtered_device with ids, a bool mask and None; Mi355xSearcher.search(graph_filter=True) on a bundle
    that stores its embeddings (the pruned bundle needs the encoder: tests/test_gpu_filtered_search.py); the ValueError cases."""
    import tempfile

    from leann_amd._compat import BACKEND_REGISTRY
    from leann_amd.backend import write_leann_bundle

    W = world("ip64")
    q = W.queries(4, 86)
    k, ef = 10, 64
    mask = half(W, 9)
    el, ed, _, _ = W.R.expected(q, k, mask, ef)
    ul, ud, _, _ = W.R.expected(q, k, None, ef)
    idx, _ = open_index(be, W)
    prm = idx.make_params(ef=ef)
    for allowed, (wl, wd) in ((np.flatnonzero(mask), (el, ed)), (mask, (el, ed)), (None, (ul, ud))):
        d, l = idx.search_filtered(q, k, prm, allowed=allowed)
        assert d.shape == (4, k) and d.dtype == np.float32 and l.dtype == np.int64 and fr.same(l, d, wl, wd)
        if not be.emulated:
            import torch

            for a in (allowed, None if allowed is None else torch.from_numpy(fr.bitmap(mask).view(np.int32)).cuda()):
                dd, ll = idx.search_filtered_device(torch.from_numpy(q).cuda(), k, prm, allowed=a)
                assert fr.same(ll.cpu().numpy(), dd.cpu().numpy(), wl, wd)
    assert fr.same(*idx.search(q, k, prm)[::-1], ul, ud)
    idx.close()
    print("index wrappers: ok", flush=True)
    texts = [f"passage {i}" for i in range(W.n)]
    ids = [int(v) for v in np.flatnonzero(mask)]
    with tempfile.TemporaryDirectory() as td:
        p = str(Path(td) / "full.leann")
        write_leann_bundle(p, texts, W.x, "sentence-transformers/all-MiniLM-L6-v2", distance_metric="mips", M=M, efConstruction=40, is_recompute=False)
        s = BACKEND_REGISTRY["mi355x"].searcher(p)
        plain = s.search(q, k, recompute_embeddings=False, complexity=ef)
        r = s.search(q, k, recompute_embeddings=False, complexity=ef, graph_filter=True, allowed_ids=ids)
        assert all(int(lab) in set(ids) for row in r["labels"] for lab in row if lab != "-1")
        kept = [[lab for lab in row if int(lab) in set(ids)] for row in plain["labels"]]
        assert all(sum(lab != "-1" for lab in row) >= len(kr) for row, kr in zip(r["labels"], kept))
        assert [row[: len(kr)] for row, kr in zip(r["labels"], kept)] == kept  # what post-filtering keeps heads the filtered result
        r2 = s.search(q, k, recompute_embeddings=False, complexity=ef, graph_filter=True, allowed_ids=mask)
        assert r2["labels"] == r["labels"]
        assert s.search(q, k, recompute_embeddings=False, complexity=ef, graph_filter=True)["labels"] == plain["labels"]
        for kw in (dict(allowed_ids=ids), dict(exact=True, graph_filter=True, allowed_ids=ids), dict(pq_flat=True, graph_filter=True, allowed_ids=ids),
                   dict(exact=True, pq_flat=True)):
            try:
                s.search(q, k, recompute_embeddings=False, **kw)
            except ValueError:
                pass
            else:
                raise AssertionError(f"{kw} must raise ValueError")
        s.cleanup()
    print("searcher wiring: ok", flush=True)


CASES["wiring"] = case_wiring


def main(argv):
    _load(argv[1])
    be = HostBackend()
    for name in argv[2:] or list(CASES):
        CASES[name](be)
    print("ALL CASES OK", flush=True)


if __name__ == "__main__":
    main(sys.argv)
