"""lm_graph_insert_batch on the MI355X: one insert batch or refinement step of the batched HNSW builder as one library call on a view
index, against tests/insert_ref/lm_insert_ref.c -- candidates, candidate distances (as bit patterns), keep masks and the three level arrays
byte for byte, the statistics those of the separate view search that supplies S.  The scenarios (tests/insert_ref_util.py: EDGE_CASES,
shared with the CPU run against the host build of the library) run over d = 64 / 96, both metrics, fp32 and fp16 tables, on the
2000-point three-level graph with caps 16 / 8 / 8, holes and an out-of-range slot; then the rejections, and the builder's opt-in path
against its torch path.  Every comparison is exact."""
import numpy as np
import pytest

from tests.util import clustered, queries_near, recall_at_k

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """(the restatement, the device)."""
    import torch

    from leann_amd import _lib
    from oracle import oracle as orc
    from tests.insert_ref_util import compile_ref, load_ref

    _lib.require_gpu()
    orc.lib()  # the restatement links against the oracle library (built on first use)
    return load_ref(compile_ref(tmp_path_factory.mktemp("insert_ref"))), torch.device("cuda", 0)


CASE_NAMES = ["insert_300", "refine_257", "refine_k512", "twin_rows", "overflow", "void_and_duplicates", "alpha", "m_above_candidates"]


def test_the_case_list_is_the_shared_one():
    from tests.insert_ref_util import EDGE_CASES

    assert list(EDGE_CASES) == CASE_NAMES


@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("d", [64, 96])
@pytest.mark.parametrize("case", CASE_NAMES)
def test_insert_batch_matches_the_c_restatement(world, case, d, metric, f16):
    """insert_300: replace = 0, 300 emptied rows nobody links to, kk = 12, m = 8.  refine_257: replace = 1 with the entry point's, the
    full, the empty and the out-of-range-slot row at K = 29, then K = 86.  refine_k512: b = 8, kk = 496 at efSearch 496.  twin_rows: two
    identical table rows -- equal distances, the position decides; rows dedupe against their stored slots and drop themselves (asserted on
    the inputs).  overflow: n = 40, efSearch 64, kk = 39, rows of 3e38 whose distances are not finite reach S and come out empty.
    void_and_duplicates: ids -1 and n + 5, one id twice.  alpha: 1.2, the relaxed pass.  m_above_candidates: m = 20 over K = 5, then the
    same handle without the optional outputs.  Statistics equal to the separate search's in every one."""
    from tests.insert_ref_util import EDGE_CASES

    ref, dev = world
    print(EDGE_CASES[case](ref, dev, d, metric, f16))


def test_rejections_touch_nothing_and_an_empty_batch_writes_nothing(world):
    """Every rejection of the header: its code, and the pre-filled level arrays and optional outputs byte for byte afterwards; b == 0 is
    LM_OK and writes nothing.  Nothing here launches."""
    from tests.insert_ref_util import case_rejections

    ref, dev = world
    for d, metric, f16 in ((64, 1, False), (96, 0, True)):
        print(case_rejections(ref, dev, d, metric, f16))


@pytest.mark.parametrize("metric", ["mips", "l2"])
def test_builder_with_the_insert_kernel_builds_the_same_graph(world, metric):
    """build_graph_gpu at 3000 x 32 (M = 8, ef_construction = 40; selector, linker, search = kernel, kernel, view): inserter="kernel"
    returns the CSR arrays of inserter="torch" byte for byte, one library call per insert batch and refinement step and no
    _LevelView.search; the graph is a good one (recall@10 >= 0.97 at ef 64: the builder quality bar of tests/test_gpu_link_kernel.py)."""
    import torch

    from leann_amd.index import Mi355xIndex
    from oracle import oracle as orc
    from tests.insert_ref_util import build_both, csr_equal

    x = clustered(3000, 32, 8, n_centers=20, sigma=0.5)
    q = queries_near(x, 100, 9)
    gt, _ = orc.bruteforce_topk(x, q, 10, 1 if metric == "l2" else 0)
    g_torch, g_kernel, counts = build_both(torch.from_numpy(x).cuda(), metric, 2048)
    g_kernel.validate()
    assert csr_equal(g_torch, g_kernel)
    assert counts["kernel"][0] == 0 and counts["kernel"][1] >= 3 and counts["torch"] == [counts["kernel"][1], 0], counts
    idx = Mi355xIndex.from_csr(g_kernel)
    idx.attach_table(x)
    _, l = idx.search(q, 10, idx.make_params(ef=64, recompute=False))
    r = recall_at_k(l, gt)
    print(f"inserter=kernel {metric}: recall@10 at ef 64 = {r:.4f}, {g_kernel.neighbors.shape[0]} links, {counts['kernel'][1]} insert calls")
    assert r >= 0.97
    idx.close()


def test_backend_parameter_reaches_the_builder(world, monkeypatch):
    """build_params["gpu_insert_kernel"]=True hands the GPU builder inserter="kernel" (with the three parameters it needs) and the graph
    equals the one the same parameters build without it."""
    from leann_amd import backend
    from leann_amd import gpu_graph_build as gb
    from tests.insert_ref_util import csr_equal

    seen = []
    real = gb.build_graph_gpu

    def recording(x, metric, **kw):
        seen.append(kw.get("inserter"))
        return real(x, metric, **kw)

    monkeypatch.setattr(gb, "build_graph_gpu", recording)
    data = clustered(2600, 32, 4, n_centers=12, sigma=0.5)
    kw = dict(M=8, efConstruction=40, gpu_build_threshold=1000, gpu_select_kernel=True, gpu_link_kernel=True, gpu_search_view=True)
    g0 = backend.Mi355xBuilder(**kw)._build_graph(data, "l2")
    g1 = backend.Mi355xBuilder(gpu_insert_kernel=True, **kw)._build_graph(data, "l2")
    assert seen == [None, "kernel"] and csr_equal(g0, g1)
