"""lm_graph_add_links on the MI355X: adj, dist (as bit patterns) and deg byte for byte against the C restatement
(tests/link_ref/lm_link_ref.c) on real traffic -- both directions of every point's search result over 20 000 points, hubs far above
LM_LINK_STAGE -- and on the edge-case set of the CPU suite; the batched builder with linker="kernel" against linker="torch"; the backend's
gpu_link_kernel build parameter end to end."""
import numpy as np
import pytest

from tests.util import clustered, queries_near, recall_at_k

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_():
    import torch

    from leann_amd import _lib

    _lib.require_gpu()
    return torch


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    from oracle import oracle as orc
    from tests.link_ref_util import compile_ref, load_ref

    orc.lib()  # the restatement links against the oracle library (built on first use)
    return load_ref(compile_ref(tmp_path_factory.mktemp("link_ref")))


def _gpu_link(torch, table, adj, dist, deg, src, dst, w, metric, alpha):
    """lm_graph_add_links on device copies of the numpy arrays -> (adj, dist, deg) as numpy."""
    from leann_amd import _lib

    lib = _lib.load()
    dev = torch.device("cuda", 0)
    t = torch.from_numpy(np.ascontiguousarray(table)).to(dev)
    a, d, g = (torch.from_numpy(np.array(v, order="C")).to(dev) for v in (adj, dist, deg))
    s, e, ww = (torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (src, dst, w))
    assert a.dtype == torch.int32 and d.dtype == torch.float32 and g.dtype == torch.int32 and s.dtype == torch.int32 and e.dtype == torch.int32 and ww.dtype == torch.float32
    n, cap = a.shape
    need = int(lib.lm_graph_add_links_workspace_bytes(n, s.shape[0]))
    ws = torch.empty((max(need, 1),), dtype=torch.uint8, device=dev)
    rc = lib.lm_graph_add_links(t.data_ptr(), _lib.DTYPE_F16 if t.dtype == torch.float16 else _lib.DTYPE_F32, t.shape[1], metric, a.data_ptr(), d.data_ptr(),
                                g.data_ptr(), n, cap, s.data_ptr(), e.data_ptr(), ww.data_ptr(), s.shape[0], alpha, ws.data_ptr(), need,
                                torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, "lm_graph_add_links")
    torch.cuda.synchronize()
    return a.cpu().numpy(), d.cpu().numpy(), g.cpu().numpy()


@pytest.mark.parametrize("metric", ["mips", "l2"])
@pytest.mark.parametrize("d", [96, 384])
def test_kernel_matches_the_c_restatement_on_real_traffic(ref, torch_, d, metric):
    """20 000 clustered points, a graph of them from build_graph_gpu, its level-0 lists laid out densely at cap 32; the edges are both
    directions of every point's k = 32 stored-table search result (~1.3 M edges; the most popular nodes collect far more than
    LM_LINK_STAGE).  alpha in {1, 1.2}, fp32 and fp16 tables: all three arrays equal the restatement's."""
    torch = torch_
    from leann_amd import _lib
    from leann_amd.gpu_graph_build import build_graph_gpu
    from leann_amd.index import Mi355xIndex
    from tests.link_ref_util import ref_link, same_bytes
    from tests.select_ref_util import pad64

    n, k, cap = 20000, 32, 32
    mt = 1 if metric == "l2" else 0
    x = clustered(n, d, 40 + d, n_centers=20, sigma=1.0)  # few, wide clusters: popular nodes (exact 32-NN in-degree up to ~400 at d = 96, ~550 at 384)
    g = build_graph_gpu(torch.from_numpy(x).cuda(), metric, M=16, ef_construction=100)
    # level-0 lists, dense [n, cap]; their distances are filled per table below
    p0 = g.node_offsets[:-1].astype(np.int64)
    beg = g.level_ptr[p0].astype(np.int64)
    deg0 = np.minimum(g.level_ptr[p0 + 1].astype(np.int64) - beg, cap)
    col = np.arange(cap)[None, :]
    m = col < deg0[:, None]
    adj = np.full((n, cap), -1, np.int32)
    adj[m] = g.neighbors[(beg[:, None] + col)[m]]
    rows = np.broadcast_to(np.arange(n, dtype=np.int32)[:, None], adj.shape)
    from tests.link_ref_util import pair_dists

    for f16 in (False, True):
        tab = x.astype(np.float16) if f16 else x
        idx = Mi355xIndex.from_csr(g)
        idx.attach_table(tab)
        dd, ids = idx.search_device(torch.from_numpy(x).cuda(), k, idx.make_params(ef=64, beam=2, recompute=False, max_batch=16384))
        torch.cuda.synchronize()
        idx.close()
        ids, dd = ids.cpu().numpy().astype(np.int32), dd.cpu().numpy()
        wi = (-dd if mt == 0 else dd).astype(np.float32)  # internal distance
        ok = (ids >= 0) & (ids != rows[:, :1])
        s, t, w = rows[:, :1].repeat(k, 1)[ok], ids[ok], wi[ok]
        src, dst, ww = np.concatenate([s, t]), np.concatenate([t, s]), np.concatenate([w, w])
        ptab = pad64(tab)
        dist = np.full((n, cap), np.inf, np.float32)
        dist[m] = pair_dists(ref, ptab, rows[m], adj[m], mt)
        deg = np.full(n, -77, np.int32)
        incoming = np.bincount(src, minlength=n)
        print(f"d={d} {metric} f16={f16}: {src.shape[0]} edges, largest bucket {incoming.max()}, rows above LM_LINK_STAGE: {int((incoming > _lib.LINK_STAGE).sum())}")
        assert src.shape[0] > 1_200_000 and incoming.max() > 2 * _lib.LINK_STAGE
        for alpha in (1.0, 1.2):
            got = _gpu_link(torch, ptab, adj, dist, deg, src, dst, ww, mt, alpha)
            exp = ref_link(ref, ptab, adj, dist, deg, src, dst, ww, mt, alpha)
            bad = np.nonzero((got[0] != exp[0]).any(1) | (got[1].view(np.uint32) != exp[1].view(np.uint32)).any(1) | (got[2] != exp[2]))[0]
            print(f"d={d} {metric} f16={f16} alpha={alpha}: mean degree {got[2].mean():.2f} (restatement {exp[2].mean():.2f}), rows that differ: {bad.shape[0]}")
            assert bad.shape[0] == 0 and same_bytes(got, exp), (d, metric, f16, alpha, bad[:10])


@pytest.mark.parametrize("metric", [0, 1])
def test_edge_case_set_on_the_gpu(ref, torch_, metric):
    """The kernel_vs_restatement edge set of tests/emulated_link_cases.py (tests.link_ref_util.edge_case_inputs) once more at n = 3000:
    untouched rows, every candidate count around cap and 2 cap, a hub of 3 x LM_LINK_STAGE edges, duplicates against existing links and among
    the edges, invalid ids, holes, NaN and -0.0 weights, garbage in d_deg; the call repeated; the edges reordered."""
    torch = torch_
    from leann_amd import _lib
    from tests.emulated_link_cases import _table
    from tests.link_ref_util import edge_case_inputs, order_preserving_permutation, ref_link, same_bytes

    n = 3000
    run = 0
    for cap, d, f16, alpha in ((1, 48, False, 1.2), (4, 384, True, 1.0), (32, 48, True, 1.2), (64, 384, False, 1.0), (_lib.SELECT_MAX_K // 2, 48, False, 1.2),
                               (_lib.SELECT_MAX_K // 2, 384, True, 1.0)):
        table = _table(n, d, 700 + run + 10 * metric, f16)
        inp = edge_case_inputs(ref, table, cap, metric, 800 + run + 10 * metric, _lib.LINK_STAGE)
        args = (inp["adj"], inp["dist"], inp["deg"], inp["src"], inp["dst"], inp["w"], metric, alpha)
        got = _gpu_link(torch, table, *args)
        exp = ref_link(ref, table, *args)
        u = inp["untouched"]
        print(f"cap={cap} d={d} metric={metric} f16={f16} alpha={alpha}: {inp['src'].shape[0]} edges")
        assert same_bytes(got, exp), (cap, d, f16, alpha)
        assert got[0][u].tobytes() == inp["adj"][u].tobytes() and got[1][u].tobytes() == inp["dist"][u].tobytes() and got[2][u].tobytes() == inp["deg"][u].tobytes()
        assert same_bytes(_gpu_link(torch, table, *args), got)
        o = order_preserving_permutation(inp["src"], inp["dst"], np.random.default_rng(run))
        assert same_bytes(_gpu_link(torch, table, inp["adj"], inp["dist"], inp["deg"], inp["src"][o], inp["dst"][o], inp["w"][o], metric, alpha), got)
        run += 1


def test_builder_gives_the_same_graph_with_either_linker(torch_):
    """build_graph_gpu on 20 000 x 96, M = 16, efc = 100, selector="kernel": byte-identical CSR arrays for linker="torch" and "kernel", and
    the quality tests/test_gpu_pipeline.py::test_gpu_graph_builder_quality asks for."""
    torch = torch_
    from leann_amd.gpu_graph_build import build_graph_gpu
    from leann_amd.index import Mi355xIndex
    from oracle import oracle as orc
    from tests.emulated_link_cases import _csr_equal

    x = clustered(20000, 96, 0, n_centers=200, sigma=0.5)
    q = queries_near(x, 200, 1)
    gt, _ = orc.bruteforce_topk(x, q, 10, 0)
    xd = torch.from_numpy(x).cuda()
    gk = build_graph_gpu(xd, "mips", M=16, ef_construction=100, selector="kernel", linker="kernel")
    g0 = build_graph_gpu(xd, "mips", M=16, ef_construction=100, selector="kernel", linker="torch")
    gk.validate()
    assert gk.level0_degrees().max() <= 32
    assert _csr_equal(gk, g0)
    idx = Mi355xIndex.from_csr(gk)
    idx.attach_table(x)
    _, l = idx.search(q, 10, idx.make_params(ef=64, recompute=False))
    r = recall_at_k(l, gt)
    print(f"linker=kernel: recall@10 at ef 64 = {r:.4f}, mean level-0 degree {gk.level0_degrees().mean():.2f}")
    assert r >= 0.97


def test_backend_build_parameter_selects_the_link_kernel(torch_, tmp_path, monkeypatch):
    """build_params["gpu_link_kernel"]=True (with gpu_select_kernel and hub_preserving_m): the GPU builder and the hub-preserving pruning
    both insert their links with lm_graph_add_links (counted) and never run the torch form; the searcher opens and searches the index."""
    from leann_amd import gpu_graph_build as gb
    from leann_amd._compat import BACKEND_REGISTRY
    from leann_amd.backend import write_leann_bundle

    calls = {"kernel": 0, "torch": 0}
    real_kernel, real_torch = gb._LevelGraph._add_links_kernel, gb._LevelGraph._add_links_torch

    def counting_kernel(self, *a, **k):
        calls["kernel"] += 1
        return real_kernel(self, *a, **k)

    def counting_torch(self, *a, **k):
        calls["torch"] += 1
        return real_torch(self, *a, **k)

    monkeypatch.setattr(gb._LevelGraph, "_add_links_kernel", counting_kernel)
    monkeypatch.setattr(gb._LevelGraph, "_add_links_torch", counting_torch)
    n = 3000
    x = clustered(n, 384, 33)
    texts = [f"passage {i}" for i in range(n)]
    p = str(tmp_path / "k.leann")
    write_leann_bundle(p, texts, x, "sentence-transformers/all-MiniLM-L6-v2", distance_metric="l2", M=8, efConstruction=40, is_recompute=False,
                       gpu_build_threshold=n, gpu_select_kernel=True, gpu_link_kernel=True, hub_preserving_m=6)
    assert calls["kernel"] > 0 and calls["torch"] == 0
    s = BACKEND_REGISTRY["mi355x"].searcher(p)
    r = s.search(x[:9] + 1e-4, 3, complexity=32, recompute_embeddings=False)
    assert [row[0] for row in r["labels"]] == [str(i) for i in range(9)]
    s.cleanup()
    # without the parameter the torch form runs, as before
    calls.update(kernel=0, torch=0)
    write_leann_bundle(str(tmp_path / "t.leann"), texts, x, "sentence-transformers/all-MiniLM-L6-v2", distance_metric="l2", M=8, efConstruction=40,
                       is_recompute=False, gpu_build_threshold=n, gpu_select_kernel=True, hub_preserving_m=6)
    assert calls["kernel"] == 0 and calls["torch"] > 0
