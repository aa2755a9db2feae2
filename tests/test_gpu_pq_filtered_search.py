"""lm_pq_batch_search_filtered (csrc/lm_pq_impl.h: k_pq_traverse<NTH, true>) on the MI355X: the cases of tests/emulated_pq_filtered_cases.py --
every mode and allow-list form at all three workgroup widths, the collecting threshold, the staging overflow, the degenerate graphs, ties /
NaN / the zero query, the three invariants of include/leann_mi355x.h (two passes among them), the LDS envelope, the rejections on
sentinel-filled buffers, the wrappers -- and a bundle with PQ codes searched through Mi355xDiskannSearcher.search(graph_filter=True,
allowed_ids=...).  Every comparison is exact: labels, distance bits, stats, the provider's request lists and "filtered_allowed_evals" against
the reference composed from the unmodified oracle in tests/pq_filtered_ref_util.py."""
import numpy as np
import pytest

from tests import emulated_pq_filtered_cases as cases


def _has_gpu() -> bool:
    try:
        import torch

        return torch.cuda.is_available()
    except Exception:  # noqa: BLE001
        return False


pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not _has_gpu(), reason="needs an MI355X")]


@pytest.fixture(scope="module")
def gpu():
    from leann_amd import _lib
    from oracle import oracle as orc

    _lib.require_gpu()
    orc.lib()
    return cases.GpuBackend()


@pytest.mark.parametrize("name", cases.LAYOUTS_A)
def test_modes_and_allow_lists(gpu, name):
    """n = 600, 9 queries, k = 10, L = 40, W = 4, both metrics; PQ order at 1024 / 512 / 256 threads, deferred, fp32 and fp16 table; nine lists."""
    cases.case_modes_and_allow_lists(gpu, (name,))


def test_the_collecting_threshold_is_the_allowed_lists_own(gpu):
    cases.case_collecting_threshold(gpu)


def test_staging_overflow_takes_several_rounds(gpu):
    cases.case_staging_overflow(gpu)


def test_degenerate_graphs(gpu):
    cases.case_degenerate_graphs(gpu)


def test_ranking_ties_nan_and_the_zero_query(gpu):
    cases.case_ranking(gpu)


def test_invariants(gpu):
    """70 queries together and alone, host and device entry, calls in a row, lm_pq_batch_search before and after, "pq_rerank_expanded", the
    HNSW search on the same handle."""
    cases.case_invariants(gpu)


def test_two_passes(gpu):
    cases.case_two_passes(gpu)


def test_lds_envelope_largest_l_and_the_next_refused(gpu):
    cases.case_lds_envelope(gpu)


def test_rejections_leave_the_outputs_untouched(gpu):
    cases.case_rejections(gpu)


def test_index_wrappers_and_backend_wiring(gpu):
    cases.case_wiring(gpu)


def test_graph_filter_on_a_bundle_with_pq_codes(tmp_path):
    """A DiskANN-style bundle of 500 passages served by Mi355xDiskannSearcher: search(graph_filter=True, allowed_ids=10 % of the ids) returns
    only allowed labels and the plain search's ndis / nexpand / nrounds; without allowed_ids it is the plain search.  In PQ order
    (skip_search_reorder) the allowed entries of the plain search's final list are the best allowed nodes the walk evaluated, so the filtered
    result has at least as many hits per query as post-filtering, those first, and more on at least one query.  After the exact rerank a node
    outside the final list may rank between them, so there the count and the labels' membership are what is certain."""
    from leann_amd._compat import BACKEND_REGISTRY
    from leann_amd.backend import write_leann_bundle
    from tests.util import clustered, queries_near

    n, k, L = 500, 10, 32
    x = clustered(n, 64, 41, n_centers=16)
    q = queries_near(x, 8, 42)
    texts = [f"passage {i}" for i in range(n)]
    p = str(tmp_path / "dk.leann")
    write_leann_bundle(p, texts, x, "sentence-transformers/all-MiniLM-L6-v2", backend_name="mi355x_diskann", distance_metric="mips")
    s = BACKEND_REGISTRY["mi355x_diskann"].searcher(p)
    allowed = set(int(v) for v in np.random.default_rng(3).permutation(n)[: n // 10])
    with pytest.raises(ValueError):
        s.search(q, k, allowed_ids=sorted(allowed))
    with pytest.raises(ValueError):
        s.search(q, k, pq_flat=True, graph_filter=True, allowed_ids=sorted(allowed))
    more = 0
    for kw in (dict(skip_search_reorder=True), dict()):
        plain = s.search(q, k, complexity=L, beam_width=2, **kw)
        st_plain = s.last_stats()
        kept = [[lab for lab in row if int(lab) in allowed] for row in plain["labels"]]
        r = s.search(q, k, complexity=L, beam_width=2, graph_filter=True, allowed_ids=sorted(allowed), **kw)
        st = s.last_stats()
        got = [[lab for lab in row if lab != "-1"] for row in r["labels"]]
        assert all(int(lab) in allowed for row in got for lab in row)
        assert all(len(g) >= len(kr) for g, kr in zip(got, kept))
        assert all(int(st[f]) == int(st_plain[f]) for f in ("ndis", "nexpand", "nrounds"))
        if kw:
            assert all(g[: len(kr)] == kr for g, kr in zip(got, kept))
            more = sum(len(g) for g in got) - sum(len(kr) for kr in kept)
        assert s.search(q, k, complexity=L, beam_width=2, graph_filter=True, **kw)["labels"] == plain["labels"]
    assert more > 0
    s.cleanup()
