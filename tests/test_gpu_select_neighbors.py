"""lm_select_neighbors on the MI355X: keep masks byte for byte against the C restatement (tests/select_ref/lm_select_ref.c, distance
function = the oracle's orc_dist) on real search output over 20 000 points; the batched builder with selector="kernel" at the quality
threshold the torch selector is held to; the backend's gpu_select_kernel build parameter end to end."""
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
    from tests.select_ref_util import compile_ref, load_ref

    orc.lib()  # the restatement links against the oracle library (built on first use)

    return load_ref(compile_ref(tmp_path_factory.mktemp("select_ref")))


@pytest.mark.parametrize("metric", ["mips", "l2"])
@pytest.mark.parametrize("d", [96, 384])
def test_kernel_matches_the_c_restatement_on_search_output(ref, torch_, d, metric):
    """20 000 clustered points; every point's candidate row = its k = 128 search result over a graph of those points (stored-embedding
    mode, lm_index_search_device), itself blanked the way the builder's refinement does it -- an empty slot at or near the front.
    m = 32, alpha in {1, 1.2}, fp32 and fp16 tables: the kernel's keep mask equals the restatement's on every row."""
    torch = torch_
    from leann_amd import _lib
    from leann_amd.gpu_graph_build import _padded_table, build_graph_gpu, select_neighbors_kernel
    from leann_amd.index import Mi355xIndex
    from tests.select_ref_util import pad64, ref_select

    n, K, m = 20000, 128, 32
    mt = 1 if metric == "l2" else 0
    x = clustered(n, d, 40 + d, n_centers=200, sigma=0.5)
    g = build_graph_gpu(torch.from_numpy(x).cuda(), metric, M=16, ef_construction=100)
    for f16 in (False, True):
        tab = x.astype(np.float16) if f16 else x
        idx = Mi355xIndex.from_csr(g)
        idx.attach_table(tab)
        dist, ids = idx.search_device(torch.from_numpy(x).cuda(), K, idx.make_params(ef=K, beam=2, recompute=False, max_batch=16384))
        torch.cuda.synchronize()
        idx.close()
        sim = dist if mt == 0 else -dist  # larger is closer: what the builder hands its selector
        selfm = ids == torch.arange(n, device=ids.device)[:, None]
        ids = ids.masked_fill(selfm, -1)
        sim = sim.masked_fill(selfm, -float("inf"))
        assert int((ids >= 0).sum(1).min()) > K // 2  # real, well filled rows
        dtab = _padded_table(torch.from_numpy(tab).cuda())
        assert dtab.dtype == (torch.float16 if f16 else torch.float32) and dtab.shape[1] % 64 == 0
        cand_h, dist_h = ids.cpu().numpy().astype(np.int32), (-sim).cpu().numpy()
        for alpha in (1.0, 1.2):
            got = select_neighbors_kernel(dtab, ids, sim, m, mt, alpha).cpu().numpy().astype(np.uint8)
            exp = ref_select(ref, pad64(tab), cand_h, dist_h, m, mt, alpha)
            bad = np.nonzero((got != exp).any(1))[0]
            print(f"d={d} {metric} f16={f16} alpha={alpha}: kept/row {got.sum() / n:.2f} (restatement {exp.sum() / n:.2f}), rows that differ: {bad.shape[0]}")
            assert bad.shape[0] == 0, (d, metric, f16, alpha, bad[:10])
            assert int(got.sum(1).max()) <= m and not bool(got[cand_h < 0].any())
    assert _lib.SELECT_MAX_K >= 256


def test_gpu_graph_builder_quality_with_the_kernel_selector(torch_):
    """tests/test_gpu_pipeline.py::test_gpu_graph_builder_quality -- same data, parameters and threshold -- with selector="kernel"."""
    torch = torch_
    from leann_amd.gpu_graph_build import build_graph_gpu
    from leann_amd.index import Mi355xIndex
    from oracle import oracle as orc

    x = clustered(20000, 96, 0, n_centers=200, sigma=0.5)
    q = queries_near(x, 200, 1)
    gt, _ = orc.bruteforce_topk(x, q, 10, 0)
    g = build_graph_gpu(torch.from_numpy(x).cuda(), "mips", M=16, ef_construction=100, selector="kernel")
    g.validate()
    assert g.level0_degrees().max() <= 32
    idx = Mi355xIndex.from_csr(g)
    idx.attach_table(x)
    _, l = idx.search(q, 10, idx.make_params(ef=64, recompute=False))
    r = recall_at_k(l, gt)
    print(f"selector=kernel: recall@10 at ef 64 = {r:.4f}, mean level-0 degree {g.level0_degrees().mean():.2f}")
    assert r >= 0.97


def test_backend_build_parameter_selects_the_kernel(torch_, tmp_path, monkeypatch):
    """build_params["gpu_select_kernel"]=True with gpu_build_threshold lowered to the corpus size: the GPU builder and the hub-preserving
    pruning both run lm_select_neighbors (counted), and the searcher opens and searches the index they wrote."""
    from leann_amd import gpu_graph_build as gb
    from leann_amd._compat import BACKEND_REGISTRY
    from leann_amd.backend import write_leann_bundle

    calls = {"kernel": 0, "torch": 0}
    real_kernel, real_torch = gb.select_neighbors_kernel, gb._select_heuristic

    def counting_kernel(*a, **k):
        calls["kernel"] += 1
        return real_kernel(*a, **k)

    def counting_torch(*a, **k):
        calls["torch"] += 1
        return real_torch(*a, **k)

    monkeypatch.setattr(gb, "select_neighbors_kernel", counting_kernel)
    monkeypatch.setattr(gb, "_select_heuristic", counting_torch)
    n = 3000
    x = clustered(n, 384, 33)
    texts = [f"passage {i}" for i in range(n)]
    p = str(tmp_path / "k.leann")
    write_leann_bundle(p, texts, x, "sentence-transformers/all-MiniLM-L6-v2", distance_metric="l2", M=8, efConstruction=40, is_recompute=False,
                       gpu_build_threshold=n, gpu_select_kernel=True, hub_preserving_m=6)
    assert calls["kernel"] > 0 and calls["torch"] == 0
    s = BACKEND_REGISTRY["mi355x"].searcher(p)
    r = s.search(x[:9] + 1e-4, 3, complexity=32, recompute_embeddings=False)
    assert [row[0] for row in r["labels"]] == [str(i) for i in range(9)]
    s.cleanup()
    # without the parameter the torch selector runs, as before
    calls.update(kernel=0, torch=0)
    write_leann_bundle(str(tmp_path / "t.leann"), texts, x, "sentence-transformers/all-MiniLM-L6-v2", distance_metric="l2", M=8, efConstruction=40,
                       is_recompute=False, gpu_build_threshold=n)
    assert calls["kernel"] == 0 and calls["torch"] > 0
