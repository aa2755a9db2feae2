"""lm_graph_prune_hubs on the MI355X: adj, dist bits, deg, hubs and indeg byte for byte against the C restatement
(tests/prune_ref/lm_prune_ref.c, which ends in the unchanged tests/link_ref/lm_link_ref.c) on the edge-case set at n = 3000 and on a
graph the GPU builder made over 20 000 points; the backend's gpu_prune_kernel build parameter end to end; search quality of the graph
pruned by the kernel against the one pruned by the host form."""
import numpy as np
import pytest

from tests.util import clustered, queries_near, recall_at_k

pytestmark = pytest.mark.gpu

N, M, D0 = 20000, 16, 96


@pytest.fixture(scope="module")
def torch_():
    import torch

    from leann_amd import _lib

    _lib.require_gpu()
    return torch


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    from oracle import oracle as orc
    from tests.prune_ref_util import compile_ref, load_ref

    orc.lib()  # the restatement links against the oracle library (built on first use)
    return load_ref(compile_ref(tmp_path_factory.mktemp("prune_ref")))


@pytest.fixture(scope="module")
def built(torch_):
    """The graph, built once: 20 000 points in 20 wide clusters, M = 16 (level-0 cap 32).  Ten of the unit vectors are stretched by 1.5:
    under the inner product a longer vector is close to everything, so these become the hubs hundreds of lists point at (the sequential
    host builder gives the plain data a largest in-degree of 90 and this data 891).  -> (x, graph, level-0 adjacency int32 [n, 32])."""
    from leann_amd.gpu_graph_build import build_graph_gpu

    x = clustered(N, D0, 7, n_centers=20, sigma=1.0)
    x[::2000] *= 1.5
    g = build_graph_gpu(torch_.from_numpy(x).cuda(), "mips", M=M, ef_construction=100)
    cap = 2 * M
    p0 = g.node_offsets[:-1].astype(np.int64)
    beg = g.level_ptr[p0].astype(np.int64)
    deg = g.level_ptr[p0 + 1].astype(np.int64) - beg
    col = np.arange(cap)[None, :]
    m = col < deg[:, None]
    adj = np.full((N, cap), -1, np.int32)
    adj[m] = g.neighbors[(beg[:, None] + col)[m]]
    return x, g, adj


def _kernel(torch, table, adj, m_low, n_hubs, metric, alpha):
    from leann_amd.gpu_graph_build import prune_level0_kernel

    out = prune_level0_kernel(torch.from_numpy(table).cuda(), torch.from_numpy(adj).cuda(), m_low, n_hubs, metric, alpha, return_indeg=True)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def test_edge_cases_match_the_c_restatement(ref, torch_):
    """The n = 3000 entries of tests.prune_ref_util.EDGE_RUNS (the set the emulation runs on the CPU): the star whose centre receives more
    than 3 * LM_LINK_STAGE reverse edges, holes, ids < 0 and >= n, self links, duplicated neighbours, rows short of their quota, a NaN row
    and a zero row in the table, a cut inside a group of equal in-degrees that straddles row 1024; the first of them twice."""
    from leann_amd import _lib
    from tests.prune_ref_util import EDGE_RUNS, check_star, differing, edge_case_adj, hubs_of_kind, ref_prune, table_for

    ran = 0
    for run, (n, cap, m_low, kind, d, metric, f16, alpha, star, twice) in enumerate(EDGE_RUNS):
        if n != 3000:
            continue
        table = table_for(n, d, 100 + run, f16)
        adj = edge_case_adj(n, cap, 300 + run, _lib.LINK_STAGE if star else 0)
        if star:
            check_star(adj, _lib.LINK_STAGE)
        n_hubs = hubs_of_kind(kind, adj)
        got = _kernel(torch_, table, adj, m_low, n_hubs, metric, alpha)
        exp = ref_prune(ref, table, adj, m_low, n_hubs, metric, alpha)
        diff = differing(got, exp)
        rows = int((got[0] != exp[0]).any(1).sum())
        dbits = got[1].view(np.uint32) != exp[1].view(np.uint32)
        print(f"n={n} cap={cap} m_low={m_low} n_hubs={n_hubs} ({kind}) d={d} metric={metric} f16={f16} alpha={alpha}: differing {diff or 'nothing'}, rows {rows}, "
              f"distances {int(dbits.sum())} (NaN on both sides: {int((dbits & np.isnan(got[1]) & np.isnan(exp[1])).sum())})")
        assert not diff, (run, diff)
        if twice:
            assert not differing(_kernel(torch_, table, adj, m_low, n_hubs, metric, alpha), got)
        ran += 1
    assert ran == 7


@pytest.mark.parametrize("metric", ["mips", "l2"])
@pytest.mark.parametrize("d", [96, 384])
def test_kernel_matches_the_c_restatement_on_a_built_graph(ref, torch_, built, d, metric):
    """m_low = 6, n_hubs = 400 on the built graph's level-0 lists, over a table of width d (the lists are the d = 96 graph's: the contract
    takes any adjacency), fp32 and fp16, alpha in {1, 1.2}: all five arrays equal the restatement's.  The largest in-degree is printed and
    must exceed 2 * LM_LINK_STAGE: such a node's reverse edges take the row kernel's multi-pass path."""
    from leann_amd import _lib
    from tests.prune_ref_util import differing, in_degrees, ref_prune
    from tests.select_ref_util import pad64

    x0, _, adj = built
    mt = 1 if metric == "l2" else 0
    x = x0 if d == D0 else clustered(N, d, 8, n_centers=20, sigma=1.0)
    top = int(in_degrees(adj).max())
    print(f"largest in-degree {top} (2 * LM_LINK_STAGE = {2 * _lib.LINK_STAGE})")
    assert top > 2 * _lib.LINK_STAGE
    for f16 in (False, True):
        table = pad64(x.astype(np.float16) if f16 else x)
        for alpha in (1.0, 1.2):
            got = _kernel(torch_, table, adj, 6, 400, mt, alpha)
            exp = ref_prune(ref, table, adj, 6, 400, mt, alpha)
            diff = differing(got, exp)
            rows = int(((got[0] != exp[0]) | (got[1].view(np.uint32) != exp[1].view(np.uint32))).any(1).sum())
            print(f"d={d} {metric} f16={f16} alpha={alpha}: mean degree {got[2].mean():.2f}, differing {diff or 'nothing'}, rows that differ: {rows}")
            assert not diff and rows == 0, (d, metric, f16, alpha, diff, rows)


def test_backend_build_parameter_selects_the_kernel(torch_, tmp_path, monkeypatch):
    """build_params["gpu_prune_kernel"]=True: the hub-preserving pruning runs prune_level0_kernel (counted), and the searcher opens and
    searches the index that was written; without the parameter the kernel form is not called."""
    from leann_amd import gpu_graph_build as gb
    from leann_amd._compat import BACKEND_REGISTRY
    from leann_amd.backend import write_leann_bundle

    calls = {"kernel": 0}
    real = gb.prune_level0_kernel

    def counting(*a, **k):
        calls["kernel"] += 1
        return real(*a, **k)

    monkeypatch.setattr(gb, "prune_level0_kernel", counting)
    n = 3000
    x = clustered(n, 384, 33)
    texts = [f"passage {i}" for i in range(n)]
    p = str(tmp_path / "k.leann")
    write_leann_bundle(p, texts, x, "sentence-transformers/all-MiniLM-L6-v2", distance_metric="l2", M=8, efConstruction=40, is_recompute=False,
                       gpu_build_threshold=n, gpu_prune_kernel=True, hub_preserving_m=6)
    assert calls["kernel"] == 1
    s = BACKEND_REGISTRY["mi355x"].searcher(p)
    r = s.search(x[:9] + 1e-4, 3, complexity=32, recompute_embeddings=False)
    assert [row[0] for row in r["labels"]] == [str(i) for i in range(9)]
    s.cleanup()
    calls.update(kernel=0)
    write_leann_bundle(str(tmp_path / "t.leann"), texts, x, "sentence-transformers/all-MiniLM-L6-v2", distance_metric="l2", M=8, efConstruction=40,
                       is_recompute=False, gpu_build_threshold=n, hub_preserving_m=6)
    assert calls["kernel"] == 0


def test_search_quality_against_the_torch_pruner(torch_, built):
    """The built graph pruned by both pruners (selector="kernel", linker="kernel", m_low = 6, 2 % hubs): recall@10 at ef 64 over 200
    queries.  The two forms differ in weight rounding and hub ties only (the torch form's single chunk holds all the edges at this size);
    the estimator's step is 1 / 2000."""
    torch = torch_
    from leann_amd.gpu_graph_build import prune_preserving_hubs
    from leann_amd.index import Mi355xIndex
    from oracle import oracle as orc

    x, g, _ = built
    q = queries_near(x, 200, 1)
    gt, _ = orc.bruteforce_topk(x, q, 10, 0)
    xd = torch.from_numpy(x).cuda()
    rec = {}
    for pruner in ("torch", "kernel"):
        p, hubs = prune_preserving_hubs(g, xd, M=M, m_low=6, hub_fraction=0.02, selector="kernel", linker="kernel", pruner=pruner, return_hubs=True)
        assert hubs.shape[0] == 400 and p.level0_degrees().max() <= 2 * M
        idx = Mi355xIndex.from_csr(p)
        idx.attach_table(x)
        _, l = idx.search(q, 10, idx.make_params(ef=64, recompute=False))
        idx.close()
        rec[pruner] = recall_at_k(l, gt)
        print(f"pruner={pruner}: recall@10 at ef 64 = {rec[pruner]:.4f}, mean level-0 degree {p.level0_degrees().mean():.2f}")
    assert rec["kernel"] >= rec["torch"] - 0.01
