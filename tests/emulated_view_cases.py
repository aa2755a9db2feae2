"""View-index scenarios (lm_index_create_view: an lm_index that searches fixed-capacity level adjacencies in place) run against
libleann_mi355x_emul.so (tests/hip_emul/build_emul_lib.py: the product's kernels on the CPU, a thread per lane).  Imported by
tests/test_graph_view.py and runnable:
    python -m tests.emulated_view_cases <path/to/libleann_mi355x_emul.so> [case ...]
The reference is the unmodified oracle over the CSR that the header declares the levels equivalent to (tests/view_ref_util.py), and
lm_index_search on Mi355xIndex.from_csr of that CSR: labels, distance bits, ndis, nexpand and nrounds equal."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np

CASES = {}
STAT_KEYS = ("ndis", "nexpand", "nrounds")


def _load(lib_path: str):
    from leann_amd import _lib

    _lib.LIB_PATH = Path(lib_path)
    _lib._lib = None
    return _lib.load()


def _oracle_search_fn(g, table, queries, ef, k):
    import torch

    from oracle import oracle as orc
    from tests.util import oracle_graph

    ids, dd, _ = orc.search(oracle_graph(g, g.d), queries.numpy(), k, ef=ef, beam=2, table=table.numpy())
    return torch.from_numpy(ids), torch.from_numpy(dd if g.metric_type == 0 else -dd)


_WORLDS = {}


def world(metric: int, n: int = 300, d: int = 48, caps=(16, 4)):
    """(x, levels, entry) -- a build_graph_gpu graph (the oracle as its candidate search) thinned into fixed-capacity levels."""
    key = (metric, n, d, caps)
    if key not in _WORLDS:
        import torch

        from leann_amd.gpu_graph_build import build_graph_gpu
        from tests.util import clustered
        from tests.view_ref_util import levels_from_csr

        x = clustered(n, d, 11 + metric, n_centers=10, sigma=0.5)
        g = build_graph_gpu(torch.from_numpy(x), "l2" if metric else "mips", M=6, ef_construction=30, search_fn=_oracle_search_fn, seed_nodes=64)
        assert g.max_level >= 1
        levels, entry = levels_from_csr(g, caps, np.random.default_rng(5 + metric))
        _WORLDS[key] = (x, levels, entry)
    return _WORLDS[key]


def _stats(idx):
    st = idx.stats()
    return {f: int(st[f]) for f in STAT_KEYS}


def _view(levels, n, d, metric, entry, table):
    from leann_amd.index import Mi355xIndex
    from tests.view_ref_util import as_tensors

    idx = Mi355xIndex.from_levels(as_tensors(levels), n, d, metric, entry)
    if table is not None:
        idx.attach_table(table)
    return idx


def case_view_vs_oracle():
    """metric x table dtype x beam x stop rule x (efSearch, k) x workgroup form x max_batch on a layered graph with holes, a full row, an
    empty row, an out-of-range slot value and a top level of one node: the view = the oracle on the composed CSR = lm_index_search on
    from_csr of it.  The CSR index and the oracle run once per parameter set; the four (form, max_batch) runs of the view are held to them."""
    from leann_amd.index import Mi355xIndex
    from oracle import oracle as orc
    from tests.util import queries_near
    from tests.view_ref_util import oracle_of, same_result

    nq, run = 5, 0
    for metric in (0, 1):
        x, levels, entry = world(metric)
        n, d = x.shape
        valid0 = (levels[0][1] >= 0) & (levels[0][1] < n)
        assert valid0.all(1).any() and (~valid0).all(1).any() and levels[-1][1].shape[0] == 1 and len(levels) >= 3  # a full row, an empty row, a top level of one node
        assert any(((a[:, 1:-1] < 0) & (a[:, :-2] >= 0) & (a[:, 2:] >= 0)).any() for _, a in levels)  # a hole in the middle of a row
        g, og = oracle_of(levels, n, d, metric, entry)
        q = queries_near(x, nq, 70 + metric)
        for f16 in (False, True):
            tab = x.astype(np.float16) if f16 else x
            ref_tab = tab.astype(np.float32)
            view = _view(levels, n, d, metric, entry, tab)
            info = view.info
            assert (info.max_degree0, info.max_degree_up, info.max_level, info.has_table) == (levels[0][1].shape[1], max(a.shape[1] for _, a in levels[1:]), len(levels) - 1, 1)
            assert info.n_neighbors == sum(a.size for _, a in levels)
            csr = Mi355xIndex.from_csr(g)
            csr.attach_table(tab)
            for beam in (1, 2, 4):
                for check in (0, 1):
                    for ef, k in ((16, 10), (8, 20), (1, 1)):
                        el, ed, est = orc.search(og, q, k, ef=ef, beam=beam, check_relative_distance=bool(check), table=ref_tab)
                        exp = (ed, el)
                        est = {f: int(est[f]) for f in STAT_KEYS}
                        prm = dict(ef=ef, beam=beam, check_relative_distance=bool(check), recompute=False)
                        got_csr = csr.search(q, k, csr.make_params(**prm))
                        ok = same_result(got_csr, exp) and _stats(csr) == est
                        # an empty walk cannot pass: some query fills all k slots where the graph has that many nodes to give, and the walk evaluates more than its seeds
                        ok = ok and est["ndis"] > nq and bool((el >= 0).all(1).any()) and bool(np.isfinite(ed[(el >= 0).all(1)]).all())
                        for wave in (0, 1):
                            view.set_option("persistent_wave", wave)
                            for max_batch in (0, 3):
                                got = view.search(q, k, view.make_params(max_batch=max_batch, **prm))
                                ok = ok and same_result(got, exp) and same_result(got, got_csr) and _stats(view) == est
                        print(f"view metric={metric} f16={f16} beam={beam} check={check} ef={ef} k={k} ndis={est['ndis']} nrounds={est['nrounds']}: {'ok' if ok else 'MISMATCH'}",
                              flush=True)
                        assert ok
                        run += 1
            view.close()
            csr.close()
    assert run == 2 * 2 * 3 * 2 * 3


CASES["view_vs_oracle"] = case_view_vs_oracle


def case_node_absent_from_level():
    """Upper-level slots that name nodes the level does not list (one of them the best neighbour by distance): the walk moves there, finds
    no row, and goes one level down -- the oracle over the CSR in which those nodes carry an empty list at that level.  Also an upper
    level given as the identity (d_nodes NULL, n_rows == ntotal)."""
    from oracle import oracle as orc
    from tests.util import queries_near
    from tests.view_ref_util import oracle_of, same_result

    for metric in (0, 1):
        x, levels, entry = world(metric)
        n, d = x.shape
        levels = [(nd, a.copy()) for nd, a in levels]
        q = queries_near(x, 4, 90 + metric)
        # the level below the single-node top: the entry point's row there names the queries' own nearest nodes, which the level does not list
        nodes1, adj1 = levels[-2]
        listed = set(nodes1.tolist())
        near = [int(v) for v in orc.bruteforce_topk(x, q, 3, metric)[0].reshape(-1) if int(v) not in listed]
        assert near
        r = int(np.searchsorted(nodes1, entry))
        assert nodes1[r] == entry
        adj1[r, : min(len(near), adj1.shape[1])] = near[: adj1.shape[1]]
        near = near[: adj1.shape[1]]
        g, og = oracle_of(levels, n, d, metric, entry, carry={v: len(levels) - 2 for v in near})
        view = _view(levels, n, d, metric, entry, x)
        for beam, ef, k in ((1, 12, 5), (3, 20, 8)):
            el, ed, est = orc.search(og, q, k, ef=ef, beam=beam, table=x)
            got = view.search(q, k, view.make_params(ef=ef, beam=beam, recompute=False))
            ok = same_result(got, (ed, el)) and _stats(view) == {f: int(est[f]) for f in STAT_KEYS}
            print(f"absent node metric={metric} beam={beam} ef={ef}: {'ok' if ok else 'MISMATCH'}", flush=True)
            assert ok
        view.close()
        # level 1 as an identity level: every node listed, most rows empty
        ident = np.full((n, 3), -1, np.int32)
        ident[entry, :2] = [(entry + 1) % n, (entry + 5) % n]
        ident[(entry + 5) % n, 1] = (entry + 9) % n
        lv = [levels[0], (None, ident)]
        g, og = oracle_of(lv, n, d, metric, entry)
        view = _view(lv, n, d, metric, entry, x)
        el, ed, est = orc.search(og, q, 5, ef=12, beam=2, table=x)
        ok = same_result(view.search(q, 5, view.make_params(ef=12, beam=2, recompute=False)), (ed, el)) and _stats(view) == {f: int(est[f]) for f in STAT_KEYS}
        print(f"identity upper level metric={metric}: {'ok' if ok else 'MISMATCH'}", flush=True)
        assert ok
        view.close()


CASES["node_absent_from_level"] = case_node_absent_from_level


def live_scenario(metric: int, x: np.ndarray, levels, entry: int, nq: int = 4):
    """Inputs of the live test, chosen on the CPU: queries = the vectors of target nodes; every level-0 link INTO a target is removed, so the
    first search cannot return it; the edges to add link each target with the nodes that search returns.  -> (levels with the cut level 0,
    its distance array, queries, targets)."""
    from oracle import oracle as orc

    n = x.shape[0]
    rng = np.random.default_rng(33 + metric)
    adj0 = levels[0][1].copy()
    upper = set()
    for nd, _ in levels[1:]:
        upper |= set(nd.tolist())
    targets = np.array([v for v in rng.permutation(n) if int(v) not in upper and v != entry][:nq], np.int32)
    adj0[np.isin(adj0, targets)] = -1
    dist0 = np.full(adj0.shape, np.inf, np.float32)
    for v, c in np.argwhere((adj0 >= 0) & (adj0 < n)):
        dist0[v, c] = orc.dist(x[v], x[adj0[v, c]], metric)
    return [(None, adj0)] + list(levels[1:]), dist0, np.ascontiguousarray(x[targets]), targets


def live_edges(metric: int, x: np.ndarray, labels_before: np.ndarray, targets: np.ndarray):
    """Both directions between every target and the three best nodes its query found before, with their canonical distances."""
    from oracle import oracle as orc

    src, dst = [], []
    for t, row in zip(targets, labels_before):
        for s in row[row >= 0][:3]:
            src += [int(s), int(t)]
            dst += [int(t), int(s)]
    w = np.array([orc.dist(x[s], x[t], metric) for s, t in zip(src, dst)], np.float32)
    return np.array(src, np.int32), np.array(dst, np.int32), w


def case_live_after_add_links():
    """search -> lm_graph_add_links into level 0 -> search, on one handle: each result is the oracle's over the CSR composed from the arrays as
    they are at that moment, and the two differ (after the call every query finds its target, which no link led to before)."""
    from leann_amd import _lib
    from oracle import oracle as orc
    from tests.view_ref_util import oracle_of, same_result

    lib = _lib.load()
    for metric in (0, 1):
        x, levels, entry = world(metric)
        n, d = x.shape
        levels, dist0, q, targets = live_scenario(metric, x, levels, entry)
        adj0 = levels[0][1]
        cap = adj0.shape[1]
        view = _view(levels, n, d, metric, entry, x)  # torch.from_numpy shares adj0's memory: the view reads the array the kernel below writes
        prm = view.make_params(ef=16, beam=2, recompute=False)
        k = 5
        g, og = oracle_of(levels, n, d, metric, entry)
        el, ed, est = orc.search(og, q, k, ef=16, beam=2, table=x)
        before = view.search(q, k, prm)
        ok = same_result(before, (ed, el)) and _stats(view) == {f: int(est[f]) for f in STAT_KEYS} and not np.isin(before[1], targets).any()
        src, dst, w = live_edges(metric, x, before[1], targets)
        tab = orc.pad64(x)
        deg = np.zeros(n, np.int32)
        ws = np.zeros(max(int(lib.lm_graph_add_links_workspace_bytes(n, src.shape[0])), 1), np.uint8)
        snapshot = adj0.copy()
        _lib.check(lib.lm_graph_add_links(tab.ctypes.data, _lib.DTYPE_F32, tab.shape[1], metric, adj0.ctypes.data, dist0.ctypes.data, deg.ctypes.data, n, cap,
                                          src.ctypes.data, dst.ctypes.data, w.ctypes.data, src.shape[0], 1.0, ws.ctypes.data, ws.shape[0], None), "lm_graph_add_links")
        assert not np.array_equal(snapshot, adj0)
        g2, og2 = oracle_of(levels, n, d, metric, entry)
        el2, ed2, est2 = orc.search(og2, q, k, ef=16, beam=2, table=x)
        after = view.search(q, k, prm)  # the same handle
        ok = ok and same_result(after, (ed2, el2)) and _stats(view) == {f: int(est2[f]) for f in STAT_KEYS}
        differ = int((before[1] != after[1]).any(1).sum())
        ok = ok and differ >= 1 and bool((after[1][:, 0] == targets).all())
        print(f"live metric={metric}: {src.shape[0]} edges, {differ} of {q.shape[0]} queries changed: {'ok' if ok else 'MISMATCH'}", flush=True)
        assert ok
        view.close()


CASES["live_after_add_links"] = case_live_after_add_links


def _csr_equal(a, b):
    return (a.ntotal == b.ntotal and a.entry_point == b.entry_point and a.max_level == b.max_level and a.levels.tobytes() == b.levels.tobytes()
            and a.level_ptr.tobytes() == b.level_ptr.tobytes() and a.node_offsets.tobytes() == b.node_offsets.tobytes() and a.neighbors.tobytes() == b.neighbors.tobytes())


def case_builder_view_equals_csr(metrics=("mips", "l2")):
    """build_graph_gpu at 3000 x 32, M = 8, ef_construction = 40, kernel selector and linker, both metrics: search="view" returns the CSR arrays
    of search="csr" byte for byte, and never assembles a temporary CSR (the one _assemble_csr call left is the final graph's).  The "csr" mode
    searches with the library too (from_csr + lm_index_search on host pointers: hip_search_fn's call without its torch.cuda stream)."""
    import torch

    from leann_amd import gpu_graph_build as gb
    from leann_amd.index import Mi355xIndex
    from tests.util import clustered

    def lib_search_fn(g, table, queries, ef, k):
        idx = Mi355xIndex.from_csr(g)
        try:
            idx.attach_table(table.numpy())
            dist, ids = idx.search(queries.numpy(), k, idx.make_params(ef=ef, beam=2, recompute=False, max_batch=16384))
            return torch.from_numpy(ids), torch.from_numpy(dist if g.metric_type == 0 else -dist)
        finally:
            idx.close()

    calls = [0]
    real = gb._assemble_csr

    def counting(*a, **kw):
        calls[0] += 1
        return real(*a, **kw)

    gb._assemble_csr = counting
    try:
        x = torch.from_numpy(clustered(3000, 32, 8, n_centers=20, sigma=0.5))
        for metric in metrics:
            kw = dict(M=8, ef_construction=40, selector="kernel", linker="kernel")
            calls[0] = 0
            gc = gb.build_graph_gpu(x, metric, search="csr", search_fn=lib_search_fn, **kw)
            n_csr = calls[0]
            calls[0] = 0
            gv = gb.build_graph_gpu(x, metric, search="view", **kw)
            n_view = calls[0]
            gv.validate()
            ok = _csr_equal(gc, gv) and n_view == 1 and n_csr > 5 and gv.max_level >= 1
            print(f"builder {metric}: {gv.neighbors.shape[0]} links, max level {gv.max_level}, CSR assemblies csr={n_csr} view={n_view}: {'ok' if ok else 'MISMATCH'}", flush=True)
            assert ok
    finally:
        gb._assemble_csr = real


CASES["builder_view_equals_csr"] = case_builder_view_equals_csr
CASES["builder_view_equals_csr_mips"] = lambda: case_builder_view_equals_csr(("mips",))  # (one metric per test: minutes each in the emulation)
CASES["builder_view_equals_csr_l2"] = lambda: case_builder_view_equals_csr(("l2",))


def case_argument_checking():
    """Every LM_EINVAL of creation (no handle comes back); every LM_ESTATE of "does not serve" and the LDS rule's LM_EINVAL with the output
    buffers pre-filled and compared byte for byte; both sides of the LDS bound; ntotal == 0; the builder's ValueErrors."""
    import pytest
    import torch

    from leann_amd import _lib
    from leann_amd.gpu_graph_build import build_graph_gpu
    from leann_amd.index import Mi355xIndex

    lib = _lib.load()
    n, d, cap = 40, 64, 4
    rng = np.random.default_rng(2)
    adj0 = rng.integers(0, n, (n, cap)).astype(np.int32)
    nodes1 = np.array([3, 9, 20], np.int32)
    adj1 = np.array([[9, 20], [3, -1], [-1, 3]], np.int32)
    x = rng.standard_normal((n, d)).astype(np.float32)

    def create(ntotal=n, dd=d, metric=0, lv=None, n_levels=None, entry=3, out=True, null_levels=False):
        lv = [(None, adj0.ctypes.data, n, cap), (nodes1.ctypes.data, adj1.ctypes.data, 3, 2)] if lv is None else lv
        arr = (_lib.GraphLevel * max(len(lv), 1))(*[_lib.GraphLevel(*t) for t in lv])
        h = C.c_void_p()
        rc = lib.lm_index_create_view(ntotal, dd, metric, None if null_levels else arr, len(lv) if n_levels is None else n_levels, entry, 0, C.byref(h) if out else None)
        return rc, h

    L0 = (None, adj0.ctypes.data, n, cap)
    L1 = (nodes1.ctypes.data, adj1.ctypes.data, 3, 2)
    bad = [dict(null_levels=True), dict(out=False), dict(n_levels=0), dict(n_levels=-1), dict(ntotal=-1), dict(ntotal=1 << 31), dict(dd=0), dict(dd=-4), dict(dd=7 * 64),
           dict(dd=1025), dict(metric=2), dict(metric=-1), dict(lv=[(None, adj0.ctypes.data, n, 0)]), dict(lv=[L0, (nodes1.ctypes.data, adj1.ctypes.data, 3, -2)]),
           dict(lv=[L0, (nodes1.ctypes.data, adj1.ctypes.data, -1, 2)]), dict(lv=[L0, (nodes1.ctypes.data, adj1.ctypes.data, n + 1, 2)]),
           dict(lv=[(nodes1.ctypes.data, adj0.ctypes.data, n, cap)]), dict(lv=[(None, adj0.ctypes.data, n - 1, cap)]), dict(lv=[L0, (None, adj1.ctypes.data, 3, 2)]),
           dict(lv=[(None, None, n, cap)]), dict(lv=[L0, (nodes1.ctypes.data, None, 3, 2)]), dict(entry=-1), dict(entry=n)]
    for over in bad:
        rc, h = create(**over)
        assert rc == _lib.LM_EINVAL and not h.value, (over, rc)
        with pytest.raises(ValueError):
            _lib.check(rc, "lm_index_create_view")
    # fine: an upper level of no rows with NULL arrays, an identity upper level, one level only
    for lv in ([L0, (None, None, 0, 2)], [L0, (None, adj0.ctypes.data, n, cap)], [L0]):
        rc, h = create(lv=lv)
        assert rc == _lib.LM_OK and h.value, lv
        lib.lm_index_free(h)
    print("creation checks: ok", flush=True)

    view = Mi355xIndex.from_levels([(None, torch.from_numpy(adj0)), (torch.from_numpy(nodes1), torch.from_numpy(adj1))], n, d, 0, 3)
    q = x[:3].copy()
    k = 4
    FILL_D, FILL_L = np.float32(7.5), np.int64(0x6E6E6E6E6E6E6E6E)

    def raw(fn, params, *mid, nq=3):
        dist, lab = np.full((nq, k), FILL_D, np.float32), np.full((nq, k), FILL_L, np.int64)
        rc = fn(view._h, nq, q.ctypes.data, k, *mid, dist.ctypes.data, lab.ctypes.data, C.byref(params))
        return rc, bool((dist == FILL_D).all() and (lab == FILL_L).all())

    good = dict(ef=8, beam=1, recompute=False)
    # no table yet
    assert raw(lib.lm_index_search, view.make_params(**good)) == (_lib.LM_ESTATE, True)
    assert raw(lib.lm_index_search_device, view.make_params(**good)) == (_lib.LM_ESTATE, True)
    view.attach_table(x)
    for fn in (lib.lm_index_search, lib.lm_index_search_device):
        for over in (dict(recompute=True), dict(batch_size=4), dict(prune_ratio=0.5)):
            assert raw(fn, view.make_params(**dict(good, **over))) == (_lib.LM_ESTATE, True), over
        view.set_option("persistent_table", 0)
        assert raw(fn, view.make_params(**good)) == (_lib.LM_ESTATE, True)
        view.set_option("persistent_table", 1)
        assert raw(fn, view.make_params(**dict(good, beam=65))) == (_lib.LM_EINVAL, True)
    words = np.full((n + 31) // 32, 0xFFFFFFFF, np.uint32)
    for fn in (lib.lm_index_search_filtered, lib.lm_index_search_filtered_device):
        for prm in (view.make_params(**good), view.make_params(ef=8, recompute=True)):
            assert raw(fn, prm, words.ctypes.data) == (_lib.LM_ESTATE, True)
            assert raw(fn, prm, None) == (_lib.LM_ESTATE, True)
    pqp = view.make_pq_params(complexity=8)
    for fn in (lib.lm_pq_batch_search, lib.lm_pq_batch_search_device):
        dist, lab = np.full((3, k), FILL_D, np.float32), np.full((3, k), FILL_L, np.int64)
        assert fn(view._h, 3, q.ctypes.data, k, C.byref(pqp), lab.ctypes.data, dist.ctypes.data) == _lib.LM_ESTATE and (dist == FILL_D).all() and (lab == FILL_L).all()
    for fn in (lib.lm_pq_batch_search_filtered, lib.lm_pq_batch_search_filtered_device, lib.lm_pq_flat_search, lib.lm_pq_flat_search_device):
        dist, lab = np.full((3, k), FILL_D, np.float32), np.full((3, k), FILL_L, np.int64)
        assert fn(view._h, 3, q.ctypes.data, k, C.byref(pqp), words.ctypes.data, lab.ctypes.data, dist.ctypes.data) == _lib.LM_ESTATE
        assert (dist == FILL_D).all() and (lab == FILL_L).all()
    cb, codes = np.zeros((4, 256, 16), np.float32), np.zeros((n, 4), np.uint8)
    assert lib.lm_pq_attach(view._h, 4, cb.ctypes.data, codes.ctypes.data, n) == _lib.LM_ESTATE
    off = np.arange(0, 65, 16, dtype=np.int32)
    assert lib.lm_pq_attach_chunked(view._h, 4, off.ctypes.data, cb.ctypes.data, codes.ctypes.data, n) == _lib.LM_ESTATE
    hub = np.array([1, 2], np.int32)
    assert lib.lm_index_set_hub_cache(view._h, hub.ctypes.data, 2, x.ctypes.data) == _lib.LM_ESTATE
    assert b"view" in lib.lm_last_error()
    # what keeps working: the plain search, and the exact search over the table
    dist, lab = view.search(q, k, view.make_params(**good))
    assert (lab[:, 0] >= 0).all()
    ed, el = view.search_exact(q, k)
    assert (el[:, 0] == np.arange(3)).all()
    view.close()
    print("does-not-serve checks: ok", flush=True)

    # the LDS rule, on both sides: efSearch = k = 8 -> (16 + P(maxnew)) * 8 + 4 * maxnew <= 153600.  cap0 = 2048, upper cap 2:
    # beam 6 -> maxnew 12288, P = 16384: 128 + 131072 + 49152 = 180352 > 153600 -> refused;  beam 4 -> maxnew 8192 = P: 128 + 65536 + 32768 = 98432 -> served;
    # beam 5 -> maxnew 10240, P = 16384: 128 + 131072 + 40960 = 172160 -> refused.  The exact edge, with cap0 = 1 and efSearch alone:
    # maxnew = 2 (the upper cap), P = 2: (2 ef + 2) * 8 + 8 <= 153600 <=> ef <= 9598.
    wide = np.full((n, 2048), -1, np.int32)
    wide[:, :cap] = adj0
    view = Mi355xIndex.from_levels([(None, torch.from_numpy(wide)), (torch.from_numpy(nodes1), torch.from_numpy(adj1))], n, d, 0, 3)
    view.attach_table(x)
    exp = Mi355xIndex.from_levels([(None, torch.from_numpy(adj0)), (torch.from_numpy(nodes1), torch.from_numpy(adj1))], n, d, 0, 3)
    exp.attach_table(x)
    want = exp.search(q, k, exp.make_params(ef=8, beam=4, recompute=False))
    for fn in (lib.lm_index_search, lib.lm_index_search_device):
        assert raw(fn, view.make_params(ef=8, beam=5, recompute=False)) == (_lib.LM_EINVAL, True)
        assert raw(fn, view.make_params(ef=8, beam=6, recompute=False)) == (_lib.LM_EINVAL, True)
    got = view.search(q, k, view.make_params(ef=8, beam=4, recompute=False))
    assert np.array_equal(got[1], want[1]) and got[0].tobytes() == want[0].tobytes()
    view.close()
    exp.close()
    one = np.ascontiguousarray(adj0[:, :1])
    view = Mi355xIndex.from_levels([(None, torch.from_numpy(one)), (torch.from_numpy(nodes1), torch.from_numpy(adj1))], n, d, 0, 3)
    view.attach_table(x)
    assert raw(lib.lm_index_search, view.make_params(ef=9599, beam=1, recompute=False)) == (_lib.LM_EINVAL, True)
    dist, lab = view.search(q, k, view.make_params(ef=9598, beam=1, recompute=False))
    assert (lab[:, 0] >= 0).all()
    view.close()
    print("LDS rule: ok", flush=True)

    # ntotal == 0: a valid handle, searches fill the empty values (ip: -inf, L2: +inf)
    for metric, empty in ((0, -np.inf), (1, np.inf)):
        e0 = Mi355xIndex.from_levels([(None, torch.zeros((0, 4), dtype=torch.int32))], 0, d, metric, -1)
        assert e0.info.ntotal == 0 and e0.info.max_level == 0 and e0.info.entry_point == -1
        dist, lab = e0.search(q, k, e0.make_params(ef=8, recompute=False))
        assert (lab == -1).all() and (dist == empty).all()
        e0.close()
    print("empty view: ok", flush=True)

    xt = torch.zeros((10, 8))
    with pytest.raises(ValueError):
        build_graph_gpu(xt, "mips", search="view")  # the torch linker
    with pytest.raises(ValueError):
        build_graph_gpu(xt, "mips", search="view", linker="torch", selector="kernel")
    with pytest.raises(ValueError):
        build_graph_gpu(xt, "mips", search="view", linker="kernel", search_fn=_oracle_search_fn)
    with pytest.raises(ValueError):
        build_graph_gpu(xt, "mips", search="bogus")
    with pytest.raises(ValueError):
        Mi355xIndex.from_levels([(None, torch.zeros((4, 2), dtype=torch.int64))], 4, 8, 0, 0)
    print("builder checks: ok", flush=True)


CASES["argument_checking"] = case_argument_checking


if __name__ == "__main__":
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    _load(sys.argv[1])
    import time

    import torch

    torch.set_num_threads(1)
    for name in (sys.argv[2:] or [c for c in CASES if not c.startswith("builder_view_equals_csr_")]):
        t0 = time.time()
        CASES[name]()
        print(f"[case {name}: {time.time() - t0:.1f} s]", flush=True)
    print("ALL CASES OK")
