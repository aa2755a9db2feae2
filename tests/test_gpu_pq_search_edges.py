"""The DiskANN-style search (csrc/lm_pq_impl.h: k_pq_traverse, k_pq_rerank, k_pq_mark, pq_search_pass) on the MI355X at the edges:
every compiled form of the ADC row fetch and both loops, lookup tables built from unequal / empty / short chunk lists, all nine
padded widths of the rerank with fp32 and fp16 tables, degenerate graphs, ties / NaN / inf, hops wider than one group of the
workgroup, the LDS limit from both sides, the expanded-set overflow fallback, more than 4096 queries and the workspace shared with
the HNSW search.  The cases, their inputs and the premises they assert from the graphs themselves live in
tests/emulated_pq_search_cases.py (which also runs them against the host build: tests/test_pq_search_edges.py); here they run at
the full sizes and at all three workgroup widths.  Every comparison is exact: labels, distance bits, ndis / nexpand / nrounds
against oracle/lm_oracle_pq.c and oracle/lm_oracle_diskann.c."""
import pytest

from tests import emulated_pq_search_cases as cases


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

    _lib.require_gpu()
    return cases.GpuBackend()


@pytest.mark.parametrize("layout", [lay[0] for lay in cases.LAYOUTS])
def test_every_adc_lut_and_rerank_instantiation(gpu, layout):
    """Case A: PQ order with counts at 1024 / 512 / 256 threads, deferred fetch (one call, sorted unique ids), fp32 and fp16 table
    rerank, both metrics."""
    cases.case_every_instantiation(gpu, layouts=(layout,))


def test_degenerate_graphs(gpu):
    """Case B: n = 1, n around 32 and 64, duplicates and self loops, entry point of degree 0, unreachable nodes, L = 1, L > n, k > L,
    W = 64 on a tiny list; unfilled slots -1 / +-inf."""
    cases.case_degenerate_graphs(gpu)


def test_ties_and_special_values(gpu):
    """Case C: five distinct code rows, every table row twice, the zero query under inner product, NaN and +inf coordinates."""
    cases.case_ties_and_special_values(gpu)


def test_wide_hops(gpu):
    """Case D: a second hop of more than 4096 neighbour slots and more than 4096 fresh nodes into a list that is not full (sort +
    rank_merge with no threshold), and one of exactly 4096 slots."""
    cases.case_wide_hops(gpu)


def test_lds_envelope(gpu):
    """Case E: 155648 bytes of LDS state are accepted and right, 163840 are refused with a ValueError naming the LDS, and the handle
    works afterwards."""
    cases.case_lds_envelope(gpu)


def test_expanded_set_overflow_falls_back_to_the_final_list(gpu):
    """Case F: queries that expand more than 4 L nodes under pq_rerank_expanded, beside queries that do not."""
    cases.case_expanded_overflow(gpu)


def test_passes_and_workspace_reuse(gpu):
    """Case G: 4100 queries (passes of 4096 and 4), then PQ and HNSW searches interleaved on one handle, host and device entry."""
    cases.case_passes_and_workspace(gpu)
