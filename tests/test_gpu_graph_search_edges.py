"""The graph search (lm_index_search: k_expand, k_update, k_search_table, k_uniq_count / k_uniq_emit, csrc/lm_beam_common.h) on the MI355X at
the edges: every form the launchers can reach (nine padded widths x two metrics x fp32 / fp16 rows x persistent / lock-step x 256 / 64
threads, and k_update's three row-addressing modes), both branches of the merge at both widths, beams of 64, 65 and 130, lists longer than
a wave and a workgroup, empty lists, duplicates, self loops, both stop rules, NaN / inf / -0, the LDS limits of a CSR index from both
sides, a request bitmap of three tiles, and sizes whose products overflow 32 bits.  The scenarios, their inputs and the premises asserted
from them live in tests/emulated_graph_search_cases.py (tests/test_graph_search_edges.py runs them against the host build and asserts the
premises); here they run at full size and in every world.  Every comparison is exact: labels, distance bits, ndis / nexpand / nrounds and
the provider's request list of every round against oracle/lm_oracle.c."""
import pytest

from tests import emulated_graph_search_cases as cases


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


@pytest.mark.parametrize("nch", cases.WIDTHS)
def test_every_form_the_launchers_can_reach(gpu, nch):
    """Case A at one padded width, 600 points, d = 64 nch - 3, 9 queries: all twelve worlds for both metrics."""
    done = cases.case_every_form(gpu, widths=(nch,))
    assert len(done) == 2 * (2 * 4 + 4)


def test_both_merge_branches_at_both_widths(gpu):
    """Case B: the hub chain's rounds sort and count at 64 and at 256 threads (premise asserted), in every world, one query and two."""
    cases.case_merge_branches(gpu)


@pytest.mark.parametrize("shape", [s[0] for s in cases.EDGE_SHAPES])
def test_expansion_edges(gpu, shape):
    """Case C, one shape under both metrics in every world it can take."""
    cases.assert_edge_premises()
    walked = cases.case_expansion_edges(gpu, shapes=(shape,))
    assert set(cases.PROVIDER_WORLDS) | {"lock_wg", "lock_wave"} <= walked


def test_lds_envelope_of_a_csr_index(gpu):
    """Case D on 1200 nodes."""
    cases.case_lds_envelope(gpu)


def test_dedup_over_several_tiles(gpu):
    """Case E: N = 262181, rank addressing at both widths, identity, memo, the hub cache on the tile borders."""
    cases.case_dedup_tiles(gpu)


def test_overflowing_sizes_are_refused_before_anything_is_allocated(gpu):
    """Case F.  The refused calls launch nothing."""
    cases.case_overflow_refusals(gpu)
