"""lm_graph_levels_to_csr_count / _fill and lm_graph_csr_to_level on the MI355X, byte for byte against the project's numpy assembly
(tests/csr_ref_util.py: _assemble_csr, then HnswCsr.validate()).  A scan workgroup takes CSR_TILE = 1024 items (csr_ref_util.SCAN_TILE):
ntotal = 1023 / 1025 / 2056 give one, two and three tiles of node offsets and about twice as many of pointers."""
import numpy as np
import pytest

from tests.csr_ref_util import CAPS, NTOTALS, check_case
from tests.util import clustered

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("ntotal", NTOTALS)
def test_both_directions_match_the_numpy_assembly(ntotal, cap):
    """Forward: level 0 plus upper levels of 37, 3 (one node not among the 37) and 0 rows; rows with holes, all empty, full, with values
    outside [0, ntotal).  Backward: every level by its own nodes, level 0 at half the cap with the overflow count, a level above every top."""
    import torch

    check_case(torch.device("cuda", 0), ntotal, cap)


def test_builder_with_the_csr_kernel_returns_the_same_arrays():
    """build_graph_gpu at 3000 x 32, M = 8, search="view": assembler="kernel" returns the HnswCsr arrays of "numpy" byte for byte, so does the
    kernel pruning; Mi355xIndex.from_csr of it returns the labels of the view search (from_levels on the same lists) on 16 queries, and
    that view's to_csr() is the same graph."""
    import torch

    from leann_amd import _lib
    from leann_amd import gpu_graph_build as gb
    from leann_amd.index import Mi355xIndex
    from tests.insert_ref_util import csr_equal

    _lib.require_gpu()
    x = clustered(3000, 32, 8, n_centers=20, sigma=0.5)
    xd = torch.from_numpy(x).cuda()
    kw = dict(M=8, ef_construction=40, selector="kernel", linker="kernel", search="view", inserter="kernel")
    gn, gk = gb.build_graph_gpu(xd, "l2", **kw), gb.build_graph_gpu(xd, "l2", assembler="kernel", **kw)
    gk.validate()
    assert csr_equal(gn, gk) and gk.max_level >= 1
    pn = gb.prune_preserving_hubs(gn, xd, M=8, m_low=4, pruner="kernel")
    pk = gb.prune_preserving_hubs(gn, xd, M=8, m_low=4, pruner="kernel", assembler="kernel")
    assert csr_equal(pn, pk) and pk.neighbors.shape[0] < gn.neighbors.shape[0]
    lv, no, lp, nb = gb._csr_to_device(gk, xd.device)
    levels = [(None, gb.level_from_csr_kernel(lv, no, lp, nb, 0, 16)[0])]
    for l in range(1, gk.max_level + 1):
        nodes = torch.nonzero(lv > l).flatten().to(torch.int32)
        levels.append((nodes, gb.level_from_csr_kernel(lv, no, lp, nb, l, 8, nodes)[0]))
    view = Mi355xIndex.from_levels(levels, 3000, 32, gk.metric_type, gk.entry_point)
    assert csr_equal(view.to_csr(M=8, ef_construction=40), gk)
    idx = Mi355xIndex.from_csr(gk)
    table = gb._padded_table(xd)
    labels = []
    for ix in (view, idx):
        ix.attach_table(table)
        labels.append(ix.search(x[:16] + np.float32(0.01), 10, ix.make_params(ef=64, recompute=False))[1])
        ix.close()
    assert np.array_equal(labels[0], labels[1]) and (labels[0] >= 0).all()
