"""The wide padded widths (1536, 2048, 2560, 3072, 4096: csrc/lm_wide_impl.h) on the MI355X against oracle.search / orc_dist /
oracle.bruteforce_topk: labels, distance bits and stats equal.  The shapes live in tests/emulated_wide_cases.py.  On a library without the
wide form every search, gather and scan here returns LM_EINVAL."""
import numpy as np
import pytest

from tests import emulated_wide_cases as cases
from tests.emulated_graph_search_cases import IP, L2, GpuBackend
from tests.test_gpu_graph_search_edges import _has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not _has_gpu(), reason="needs an MI355X")]


@pytest.fixture(scope="module")
def gpu():
    from leann_amd import _lib

    _lib.require_gpu()
    return GpuBackend()


@pytest.mark.parametrize("metric", (IP, L2))
@pytest.mark.parametrize("dp", cases.WIDTHS)
def test_search_at_every_wide_width(gpu, dp, metric):
    """400 nodes, d = dp - 3 and d = dp, beam 1 and 4, fp32 and fp16 tables, the persistent launch and the lock-step rounds."""
    cases.run_search(gpu, dp, metric, 400)


@pytest.mark.parametrize("metric", (IP, L2))
@pytest.mark.parametrize("dp", (1536, 4096))
def test_provider_mode(gpu, dp, metric):
    cases.run_provider(gpu, dp, metric, 400)


@pytest.mark.parametrize("npairs", (1, 17, 1000))
@pytest.mark.parametrize("metric", (IP, L2))
@pytest.mark.parametrize("f16", (False, True))
@pytest.mark.parametrize("dp", cases.WIDTHS)
def test_dist_gather(dp, f16, metric, npairs):
    from tests import gpu_abi_util as au

    tab, q, qidx, ids, exp = cases.gather_case(dp, f16, npairs, metric)
    rc, out, guard = au.dist_gather(tab, dp, metric, q, qidx, ids)
    assert rc == 0 and np.all(guard == au.FILL_F32_BITS) and np.array_equal(out.view(np.uint32), exp.view(np.uint32))


@pytest.mark.parametrize("masked", (False, True))
@pytest.mark.parametrize("nq", (1, 9))
@pytest.mark.parametrize("ntable", (1, 1500))
@pytest.mark.parametrize("dp", (1536, 2560, 4096))
def test_exact_scan(dp, ntable, nq, masked):
    """One and two slices; a second query tile and, from 2560 on, a partial sub-tile of queries; both metrics, the dtype alternating."""
    from tests import gpu_exact_util as xu

    for metric in (IP, L2):
        table, q, words, el, ed = cases.exact_case(dp, ntable, nq, bool(metric) != masked, metric, masked)
        rc, L, D, ok = xu.exact_gpu(table, q, 10, metric, words)
        assert rc == 0 and ok and xu.same(L, D, el, ed)


def test_lds_envelope_at_4096(gpu):
    cases.run_envelope(gpu, 400)


def test_refusals(gpu):
    cases.run_refusals(gpu)
