"""lm_index_create_view on the MI355X: the view of device-resident level adjacencies against the oracle over the equivalent CSR
(tests/view_ref_util.py) and against lm_index_search_device on that CSR -- labels, distance bits, ndis, nexpand, nrounds --; the search that
follows lm_graph_add_links on the same stream, on the same handle; the batched builder with search="view" against search="csr"; the
rejections."""
import ctypes as C

import numpy as np
import pytest

from tests.util import clustered, queries_near, recall_at_k

pytestmark = pytest.mark.gpu

STAT_KEYS = ("ndis", "nexpand", "nrounds")
N, ROWS, CAPS = 2000, (2000, 130, 9), (16, 8, 8)


@pytest.fixture(scope="module")
def torch_():
    import torch

    from leann_amd import _lib

    _lib.require_gpu()
    return torch


_GRAPHS = {}


def layered_graph(d: int, metric: int):
    """(x, levels, entry): 2000 clustered points on three nested levels of 2000 / 130 / 9 rows with caps 16 / 8 / 8; a row links its node to
    its nearest nodes of the level (3 .. cap - 4 of them, so that rows keep room), scattered over the slots with holes in between; one row
    per level filled to cap, one emptied, one slot holding an out-of-range value."""
    key = (d, metric)
    if key in _GRAPHS:
        return _GRAPHS[key]
    rng = np.random.default_rng(100 + d + metric)
    x = clustered(N, d, 7 + d, n_centers=16, sigma=0.6)
    sim = x @ x.T  # unit vectors: the nearest by inner product are the nearest by L2
    np.fill_diagonal(sim, -np.inf)
    order = rng.permutation(N)
    levels = []
    for l, (rows, cap) in enumerate(zip(ROWS, CAPS)):
        ids = np.sort(order[:rows]).astype(np.int32)
        adj = np.full((rows, cap), -1, np.int32)
        for r, v in enumerate(ids):
            m = int(rng.integers(3, cap - 3))
            nb = ids[np.argsort(-sim[v, ids], kind="stable")[:m]]
            adj[r, np.sort(rng.permutation(cap)[:m])] = nb
        full, empty = [int(r) for r in rng.permutation(rows) if ids[r] != order[0]][:2]  # (the entry point keeps its row)
        adj[full] = ids[np.argsort(-sim[ids[full], ids], kind="stable")[:cap]]
        adj[empty] = -1
        adj[tuple(np.argwhere(adj == -1)[0])] = N + 3
        levels.append((None if l == 0 else ids, adj))
    _GRAPHS[key] = (x, levels, int(order[0]))
    return _GRAPHS[key]


def _stats(idx):
    st = idx.stats()
    return {f: int(st[f]) for f in STAT_KEYS}


def _view(torch, levels, n, d, metric, entry, table):
    from leann_amd.gpu_graph_build import _padded_table
    from leann_amd.index import Mi355xIndex
    from tests.view_ref_util import as_tensors

    dev = torch.device("cuda", 0)
    idx = Mi355xIndex.from_levels(as_tensors(levels, dev), n, d, metric, entry)
    idx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    idx.attach_table(_padded_table(torch.from_numpy(table).to(dev)))
    return idx


def _search(torch, idx, q, k, prm):
    dist, lab = idx.search_device(torch.from_numpy(q).cuda(), k, prm)
    return dist.cpu().numpy(), lab.cpu().numpy()


@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("d", [64, 96])
def test_view_matches_the_oracle_and_the_csr_index(torch_, d, metric, f16):
    """beam 1 / 2 / 4 x efSearch 16 / 40 at k = 10 over 64 queries, both workgroup forms, max_batch 0 and 7 (ten passes, the last of one
    query): every run of the view equals the oracle and lm_index_search_device on the composed CSR."""
    torch = torch_
    from leann_amd.index import Mi355xIndex
    from oracle import oracle as orc
    from tests.view_ref_util import oracle_of, same_result

    x, levels, entry = layered_graph(d, metric)
    g, og = oracle_of(levels, N, d, metric, entry)
    q = queries_near(x, 64, 3 + d)
    tab = x.astype(np.float16) if f16 else x
    ref_tab = tab.astype(np.float32)
    view = _view(torch, levels, N, d, metric, entry, tab)
    info = view.info
    assert (info.ntotal, info.d_padded, info.max_level, info.max_degree0, info.max_degree_up, info.n_neighbors) == (N, (d + 63) // 64 * 64, 2, 16, 8, 2000 * 16 + 130 * 8 + 9 * 8)
    csr = Mi355xIndex.from_csr(g)
    csr.attach_table(tab)
    k = 10
    for beam in (1, 2, 4):
        for ef in (16, 40):
            el, ed, est = orc.search(og, q, k, ef=ef, beam=beam, table=ref_tab)
            est = {f: int(est[f]) for f in STAT_KEYS}
            assert est["ndis"] > 64 and (el >= 0).all() and np.isfinite(ed).all()  # every query fills its k slots: no empty walk passes
            got_csr = _search(torch, csr, q, k, csr.make_params(ef=ef, beam=beam, recompute=False))
            assert same_result(got_csr, (ed, el)) and _stats(csr) == est
            for wave in (0, 1):
                view.set_option("persistent_wave", wave)
                for max_batch in (0, 7):
                    got = _search(torch, view, q, k, view.make_params(ef=ef, beam=beam, recompute=False, max_batch=max_batch))
                    tag = f"beam={beam} ef={ef} wave={wave} max_batch={max_batch}"
                    assert same_result(got, (ed, el)), tag
                    assert same_result(got, got_csr), tag
                    assert _stats(view) == est, (tag, _stats(view), est)
    view.close()
    csr.close()


@pytest.mark.parametrize("metric", [0, 1])
def test_search_sees_lm_graph_add_links_without_a_new_handle(torch_, metric):
    """search -> lm_graph_add_links into level 0 on the same stream -> search, one handle: each result is the oracle's over the CSR composed
    from the arrays as they are at that moment; before the call no query can find its target (no link leads to it), after it every one does."""
    torch = torch_
    from leann_amd import _lib
    from leann_amd.gpu_graph_build import _padded_table
    from leann_amd.index import Mi355xIndex
    from oracle import oracle as orc
    from tests.emulated_view_cases import live_edges, live_scenario
    from tests.view_ref_util import as_tensors, oracle_of, same_result

    lib = _lib.load()
    d = 64
    x, levels, entry = layered_graph(d, metric)
    levels, dist0, q, targets = live_scenario(metric, x, levels, entry, nq=8)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    tl = as_tensors(levels, dev)
    adj0 = tl[0][1]
    tab = _padded_table(torch.from_numpy(x).to(dev))
    view = Mi355xIndex.from_levels(tl, N, d, metric, entry)
    view.set_stream(st)
    view.attach_table(tab)
    prm = view.make_params(ef=16, beam=2, recompute=False)
    k = 5
    g, og = oracle_of(levels, N, d, metric, entry)
    el, ed, est = orc.search(og, q, k, ef=16, beam=2, table=x)
    before = _search(torch, view, q, k, prm)
    assert same_result(before, (ed, el)) and _stats(view) == {f: int(est[f]) for f in STAT_KEYS}
    assert not np.isin(before[1], targets).any()
    src, dst, w = live_edges(metric, x, before[1], targets)
    s, e, ww = (torch.from_numpy(v).to(dev) for v in (src, dst, w))
    dd = torch.from_numpy(dist0).to(dev)
    deg = torch.zeros((N,), dtype=torch.int32, device=dev)
    need = int(lib.lm_graph_add_links_workspace_bytes(N, src.shape[0]))
    ws = torch.empty((max(need, 1),), dtype=torch.uint8, device=dev)
    _lib.check(lib.lm_graph_add_links(tab.data_ptr(), _lib.DTYPE_F32, tab.shape[1], metric, adj0.data_ptr(), dd.data_ptr(), deg.data_ptr(), N, adj0.shape[1], s.data_ptr(),
                                      e.data_ptr(), ww.data_ptr(), src.shape[0], 1.0, ws.data_ptr(), need, st), "lm_graph_add_links")
    after = _search(torch, view, q, k, prm)  # no synchronisation, no new handle: stream order alone
    now = [(None, adj0.cpu().numpy())] + list(levels[1:])
    assert not np.array_equal(now[0][1], levels[0][1])
    g2, og2 = oracle_of(now, N, d, metric, entry)
    el2, ed2, est2 = orc.search(og2, q, k, ef=16, beam=2, table=x)
    assert same_result(after, (ed2, el2)) and _stats(view) == {f: int(est2[f]) for f in STAT_KEYS}
    assert (before[1] != after[1]).any(1).all() and (after[1][:, 0] == targets).all()
    view.close()


def _csr_equal(a, b):
    return (a.ntotal == b.ntotal and a.entry_point == b.entry_point and a.max_level == b.max_level and a.levels.tobytes() == b.levels.tobytes()
            and a.level_ptr.tobytes() == b.level_ptr.tobytes() and a.node_offsets.tobytes() == b.node_offsets.tobytes() and a.neighbors.tobytes() == b.neighbors.tobytes())


@pytest.mark.parametrize("metric", ["mips", "l2"])
def test_builder_with_view_search_builds_the_csr_search_graph(torch_, metric, monkeypatch):
    """build_graph_gpu at 3000 x 32 (M = 8, ef_construction = 40, kernel selector and linker): search="view" returns the CSR arrays of
    search="csr" byte for byte without assembling a temporary CSR, and the graph is a good one (recall@10 >= 0.97 at ef 64: the builder
    quality bar of tests/test_gpu_link_kernel.py)."""
    torch = torch_
    from leann_amd import gpu_graph_build as gb
    from leann_amd.index import Mi355xIndex
    from oracle import oracle as orc

    calls = [0]
    real = gb._assemble_csr

    def counting(*a, **kw):
        calls[0] += 1
        return real(*a, **kw)

    monkeypatch.setattr(gb, "_assemble_csr", counting)
    x = clustered(3000, 32, 8, n_centers=20, sigma=0.5)
    q = queries_near(x, 100, 9)
    mt = 1 if metric == "l2" else 0
    gt, _ = orc.bruteforce_topk(x, q, 10, mt)
    xd = torch.from_numpy(x).cuda()
    kw = dict(M=8, ef_construction=40, selector="kernel", linker="kernel")
    gc = gb.build_graph_gpu(xd, metric, search="csr", **kw)
    n_csr, calls[0] = calls[0], 0
    gv = gb.build_graph_gpu(xd, metric, search="view", **kw)
    assert calls[0] == 1 and n_csr > 5  # the final graph's assembly only
    gv.validate()
    assert _csr_equal(gc, gv)
    idx = Mi355xIndex.from_csr(gv)
    idx.attach_table(x)
    _, l = idx.search(q, 10, idx.make_params(ef=64, recompute=False))
    r = recall_at_k(l, gt)
    print(f"search=view {metric}: recall@10 at ef 64 = {r:.4f}, {gv.neighbors.shape[0]} links, CSR assemblies csr={n_csr} view=1")
    assert r >= 0.97
    idx.close()


def test_rejections_touch_nothing(torch_):
    """What a view does not serve returns LM_ESTATE, the LDS rule and beam_size > 64 LM_EINVAL, each before any launch: the pre-filled device
    outputs come back byte for byte.  Creation rejects bad descriptors with no handle.  Nothing here launches a search that could fault."""
    torch = torch_
    from leann_amd import _lib
    from leann_amd.index import Mi355xIndex

    lib = _lib.load()
    d, metric = 64, 0
    x, levels, entry = layered_graph(d, metric)
    view = _view(torch, levels, N, d, metric, entry, x)
    q = torch.from_numpy(queries_near(x, 4, 5)).cuda()
    k = 5

    def refused(fn, params, *mid, pq=False):
        dist = torch.full((4, k), 7.5, dtype=torch.float32, device=q.device)
        lab = torch.full((4, k), 0x6E6E6E6E, dtype=torch.int64, device=q.device)
        outs = (C.c_void_p(lab.data_ptr()), C.c_void_p(dist.data_ptr())) if pq else (C.c_void_p(dist.data_ptr()), C.c_void_p(lab.data_ptr()))
        args = (view._h, 4, C.c_void_p(q.data_ptr()), k) + ((C.byref(params),) + mid + outs if pq else mid + outs + (C.byref(params),))
        rc = fn(*args)
        torch.cuda.synchronize()
        assert bool((dist == 7.5).all()) and bool((lab == 0x6E6E6E6E).all())
        return rc

    good = dict(ef=16, beam=1, recompute=False)
    for over in (dict(recompute=True), dict(batch_size=4), dict(prune_ratio=0.5)):
        assert refused(lib.lm_index_search_device, view.make_params(**dict(good, **over))) == _lib.LM_ESTATE, over
    view.set_option("persistent_table", 0)
    assert refused(lib.lm_index_search_device, view.make_params(**good)) == _lib.LM_ESTATE
    view.set_option("persistent_table", 1)
    assert refused(lib.lm_index_search_device, view.make_params(**dict(good, beam=65))) == _lib.LM_EINVAL
    # the LDS rule at cap0 = 16, upper cap 8: beam 64 -> maxnew 1024 = P; (2 ef + 1024) * 8 + 4096 <= 153600 <=> ef <= 8832
    assert refused(lib.lm_index_search_device, view.make_params(ef=8833, beam=64, recompute=False)) == _lib.LM_EINVAL
    assert refused(lib.lm_index_search_filtered_device, view.make_params(**good), None) == _lib.LM_ESTATE
    pqp = view.make_pq_params(complexity=16)
    assert refused(lib.lm_pq_batch_search_device, pqp, pq=True) == _lib.LM_ESTATE
    assert refused(lib.lm_pq_batch_search_filtered_device, pqp, None, pq=True) == _lib.LM_ESTATE
    assert refused(lib.lm_pq_flat_search_device, pqp, None, pq=True) == _lib.LM_ESTATE
    hub = np.array([1, 2], np.int32)
    assert lib.lm_index_set_hub_cache(view._h, hub.ctypes.data, 2, C.c_void_p(q.data_ptr())) == _lib.LM_ESTATE
    # what keeps working: the search itself, and the exact search over the table
    dist, lab = view.search_device(q, k, view.make_params(**good))
    assert bool((lab >= 0).all())
    ed, el = view.search_exact_device(q, k)
    assert bool((el >= 0).all())
    view.close()
    # creation: no handle for a level 0 that is not the identity, a zero cap, an entry point out of range
    a0 = torch.zeros((8, 4), dtype=torch.int32, device=q.device)
    nd = torch.arange(8, dtype=torch.int32, device=q.device)
    for lv, entry_ in (([(nd, a0)], 0), ([(None, a0[:, :0].contiguous())], 0), ([(None, a0)], 8), ([(None, a0)], -1)):
        with pytest.raises(ValueError):
            Mi355xIndex.from_levels(lv, 8, 64, 0, entry_)
    e0 = Mi355xIndex.from_levels([(None, a0[:0].contiguous())], 0, 64, 1, -1)
    dist, lab = e0.search_device(q, k, e0.make_params(ef=8, recompute=False))
    assert bool((lab == -1).all()) and bool(torch.isinf(dist).all())
    e0.close()
