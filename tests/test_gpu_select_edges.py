"""lm_select_neighbors on the MI355X at the shapes tests/emulated_select_cases.py runs on the CPU emulation, and at those only the
gfx950 build can get wrong: K from 1 to LM_SELECT_MAX_K (the 512-bit keep mask in registers), m >= K, row counts that leave a
workgroup -- and a wave -- partly empty, all nine padded widths (NCH = 1, 2, 3, 4, 5, 6, 8, 12, 16), alpha = 1.5, ids >= ntable, and
rows built so that the four 16-lane groups of a wave do very different amounts of work while they shuffle.  Keep masks are compared
byte for byte with the C restatement (tests/select_ref/lm_select_ref.c); the premises (ties, rows cut short by the rule, the relaxed
pass adding links) are asserted on the restatement's output, never on the kernel's."""
import functools

import numpy as np
import pytest

from tests.emulated_select_cases import _integer_rows, _table
from tests.select_ref_util import awkward_rows, internal_dist, pad64, ref_select


def _has_gpu() -> bool:
    try:
        import torch

        return torch.cuda.is_available()
    except Exception:  # noqa: BLE001
        return False


pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not _has_gpu(), reason="needs an MI355X")]

# (K, m, n): tests.emulated_select_cases.case_kernel_vs_restatement's six, K = 257 (one bit into the fifth mask word) and m > K
SHAPES = [(1, 1, 203), (7, 3, 301), (64, 12, 150), (128, 64, 37), (193, 32, 29), (512, 64, 9), (257, 64, 21), (24, 40, 17)]
COMBOS = [(metric, f16, alpha) for metric in (0, 1) for f16 in (False, True) for alpha in (1.0, 1.2, 1.5)]
WIDTHS = [64, 128, 192, 256, 320, 384, 512, 768, 1024]
DIVERGENT_N = [1, 3, 15, 17, 33, 4097]


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    from leann_amd import _lib
    from oracle import oracle as orc
    from tests.select_ref_util import compile_ref, load_ref

    _lib.require_gpu()
    orc.lib()  # the restatement links against the oracle library (built on first use)
    return load_ref(compile_ref(tmp_path_factory.mktemp("select_ref")))


def _matrix_d(si: int) -> int:
    return (48, 96, 384)[si % 3]


@functools.lru_cache(maxsize=None)
def _matrix_input(si: int, metric: int, f16: bool):
    """Table with duplicate vectors and awkward candidate rows for shape number si (the same for every alpha)."""
    K, m, n = SHAPES[si]
    seed = 100 * si + 10 * metric + int(f16)
    table = _table(max(K + 7, 300), _matrix_d(si), 1000 + seed, f16)
    cand, dist = awkward_rows(table.astype(np.float32), n, K, metric, 2000 + seed)
    return table, cand, dist


def _check_mask(got, guard, exp, cand, ntable, m, what):
    from tests.gpu_abi_util import FILL_BYTE

    assert set(np.unique(got).tolist()) <= {0, 1}, (what, np.unique(got))  # (so no 0xEE is left inside [n][K] either)
    assert (guard == FILL_BYTE).all(), what
    bad = np.nonzero((got != exp).any(1))[0]
    assert bad.shape[0] == 0, (what, bad[:10])
    valid = (cand >= 0) & (cand < ntable)
    assert not bool(got[~valid].any()) and (got.shape[0] == 0 or int(got.sum(1).max()) <= m), what


def matrix_premises(ref):
    """Over the whole shape matrix, on the restatement's output: some row keeps fewer than min(m, valid slots) -- the rule, not the cap,
    ended it --; for alpha > 1 the relaxed pass adds at least one link over alpha = 1 on the same input; ids >= ntable are present."""
    cut = relaxed = over = 0
    for si, (K, m, n) in enumerate(SHAPES):
        for metric in (0, 1):
            for f16 in (False, True):
                table, cand, dist = _matrix_input(si, metric, f16)
                valid = (cand >= 0) & (cand < table.shape[0])
                over += int((cand >= table.shape[0]).sum())
                e1 = ref_select(ref, table, cand, dist, m, metric, 1.0)
                cut += int((e1.sum(1) < np.minimum(m, valid.sum(1))).sum())
                for alpha in (1.2, 1.5):
                    ea = ref_select(ref, table, cand, dist, m, metric, alpha)
                    assert not bool((e1 & ~ea).any())  # the relaxed pass only adds
                    relaxed += int(ea.sum() - e1.sum())
    return cut, relaxed, over


def test_premises_hold_on_the_restatement(ref):
    cut, relaxed, over = matrix_premises(ref)
    print(f"rows the rule cut short: {cut}; links the relaxed pass added: {relaxed}; ids >= ntable: {over}")
    assert cut > 0 and relaxed > 0 and over > 0


@pytest.mark.parametrize("si", range(len(SHAPES)), ids=[f"K{K}-m{m}-n{n}" for K, m, n in SHAPES])
def test_kernel_matches_the_restatement_on_the_shape_matrix(ref, si):
    """Both metrics x fp32 / fp16 tables x alpha in {1, 1.2, 1.5} at every (K, m, n); the first launch of each shape is repeated."""
    from leann_amd import _lib
    from tests.gpu_abi_util import select_neighbors

    K, m, n = SHAPES[si]
    assert K <= _lib.SELECT_MAX_K == 512
    for ci, (metric, f16, alpha) in enumerate(COMBOS):
        table, cand, dist = _matrix_input(si, metric, f16)
        what = (K, m, n, table.shape[1], metric, f16, alpha)
        rc, got, guard = select_neighbors(table, cand, dist, m, metric, alpha)
        assert rc == _lib.LM_OK, what
        exp = ref_select(ref, table, cand, dist, m, metric, alpha)
        _check_mask(got, guard, exp, cand, table.shape[0], m, what)
        if ci == 0:  # the same input again: the same bytes
            rc, again, _ = select_neighbors(table, cand, dist, m, metric, alpha)
            assert rc == _lib.LM_OK and again.tobytes() == got.tobytes(), what


@pytest.mark.parametrize("dp", WIDTHS)
def test_every_padded_width(ref, dp):
    """One instantiation of k_select_neighbors per supported d_padded: (K, m, n) = (64, 12, 150), both metrics, both dtypes, alpha 1.2."""
    from leann_amd import _lib
    from tests.gpu_abi_util import select_neighbors

    K, m, n = 64, 12, 150
    d = dp - 5  # the last five columns are padding
    for f16 in (False, True):
        table = _table(300, d, 3000 + dp, f16)
        assert table.shape[1] == dp
        for metric in (0, 1):
            cand, dist = awkward_rows(table.astype(np.float32), n, K, metric, 3100 + dp + metric)
            rc, got, guard = select_neighbors(table, cand, dist, m, metric, 1.2)
            assert rc == _lib.LM_OK, (dp, f16, metric)
            _check_mask(got, guard, ref_select(ref, table, cand, dist, m, metric, 1.2), cand, table.shape[0], m, (dp, f16, metric))


@pytest.mark.parametrize("dp", [448, 640])
def test_unsupported_width_is_rejected_and_writes_nothing(ref, dp):
    from leann_amd import _lib
    from tests.gpu_abi_util import FILL_BYTE, select_neighbors

    for f16 in (False, True):
        table = _table(300, dp, 3200 + dp, f16)
        cand, dist = awkward_rows(table.astype(np.float32), 33, 16, 1, 3300 + dp)
        rc, got, guard = select_neighbors(table, cand, dist, 4, 1, 1.0)
        assert rc == _lib.LM_EINVAL and "unsupported padded dimension" in _lib.last_error()
        assert (got == FILL_BYTE).all() and (guard == FILL_BYTE).all()


def _divergent_rows(n: int, metric: int, f16: bool):
    """K = 128 rows over a 128-wide table whose neighbours in a wave do very different amounts of work: row 4i is empty, row 4i + 1 has
    one valid slot, row 4i + 2 is a full row of far-apart vectors (scaled unit vectors: no one dominates another, everything is kept up
    to m) and row 4i + 3 a full row of 128 copies of one vector under different ids (the first is kept, every other is dominated at the
    first comparison).  All values are small multiples of 1/16: exact in fp16."""
    K = 128
    x = np.zeros((2 * K + 2, 128), np.float32)
    x[np.arange(K), np.arange(K)] = 10.0 + np.arange(K) / 16.0  # 0 .. 127: far apart
    x[K : 2 * K, :64] = 2.0                                     # 128 .. 255: one vector, 128 ids
    # 256: the base of L2 rows (the origin); 257: the base of inner-product rows (all ones)
    x[2 * K + 1] = 1.0
    base = np.full(n, 2 * K + 1 if metric == 0 else 2 * K, np.int64)
    rng = np.random.default_rng(n + metric)
    cand = np.full((n, K), -1, np.int32)
    for r in range(n):
        kind = r % 4
        if kind == 1:
            slot = int(rng.integers(0, K))
            cand[r, slot] = int(rng.integers(0, K))
            if (r // 4) % 2:  # every other one also holds an id >= ntable: an empty slot like the -1s
                cand[r, (slot + 1 + int(rng.integers(0, K - 1))) % K] = x.shape[0] + 3
        elif kind == 2:
            cand[r] = np.roll(np.arange(K), r)
        elif kind == 3:
            cand[r] = K + rng.permutation(K)
    dist = internal_dist(x, base, cand, metric)
    o = np.argsort(dist, axis=1, kind="stable")  # best first, empty slots (+inf) last -- except the ids >= ntable, which keep a finite distance
    cand, dist = np.take_along_axis(cand, o, 1), np.take_along_axis(dist, o, 1)
    return (x.astype(np.float16) if f16 else x), np.ascontiguousarray(cand), np.ascontiguousarray(dist)


@pytest.mark.parametrize("n", DIVERGENT_N)
def test_divergent_groups_of_a_wave(ref, n):
    """Partial workgroups and partial waves (n = 1, 3, 15, 17, 33; 4097 = 256 workgroups and one row) with the four row kinds of
    _divergent_rows side by side in every wave, m = 32 and m = 200 > K."""
    from leann_amd import _lib
    from tests.gpu_abi_util import select_neighbors

    for metric in (0, 1):
        for f16 in (False, True):
            table, cand, dist = _divergent_rows(n, metric, f16)
            valid = ((cand >= 0) & (cand < table.shape[0])).sum(1)
            assert all(int(valid[r]) == (0, 1, 128, 128)[r % 4] for r in range(n))
            for m, alpha in ((32, 1.0), (32, 1.5), (200, 1.2)):
                exp = ref_select(ref, table, cand, dist, m, metric, alpha)
                # the premise, on the restatement: the four kinds keep 0, 1, min(m, 128) and 1
                assert all(int(exp[r].sum()) == (0, 1, min(m, 128), 1)[r % 4] for r in range(n)), (n, metric, f16, m, alpha)
                rc, got, guard = select_neighbors(table, cand, dist, m, metric, alpha)
                assert rc == _lib.LM_OK
                _check_mask(got, guard, exp, cand, table.shape[0], m, (n, metric, f16, m, alpha))


def test_three_way_on_exact_arithmetic(ref):
    """tests.emulated_select_cases.case_three_way_on_exact_arithmetic's integer data: gpu_graph_build._select_heuristic_scan (fp32 on CPU
    tensors), the C restatement and the kernel on the MI355X return the same mask; the data does hold ties at the rule's comparison."""
    import torch

    from leann_amd import _lib
    from leann_amd import gpu_graph_build as gb
    from tests.gpu_abi_util import select_neighbors

    for metric in (0, 1):
        for (N, d, n, K, m) in ((300, 48, 210, 24, 8), (200, 96, 101, 64, 16), (120, 16, 150, 32, 32), (64, 8, 99, 12, 3)):
            x, cand, dist = _integer_rows(N, d, n, K, metric, 7 * d + metric)
            a = gb._select_heuristic_scan(torch.from_numpy(x), torch.from_numpy(cand.astype(np.int64)), torch.from_numpy(-dist), m, metric).numpy().astype(np.uint8)
            for f16 in (False, True):  # small integers are exact in fp16 as well
                table = pad64(x.astype(np.float16) if f16 else x)
                b = ref_select(ref, table, cand, dist, m, metric, 1.0)
                rc, c, guard = select_neighbors(table, cand, dist, m, metric, 1.0)
                assert rc == _lib.LM_OK
                assert np.array_equal(a, b), (metric, N, d, K, m, f16)
                _check_mask(c, guard, b, cand, N, m, (metric, N, d, K, m, f16))
            v = x[np.clip(cand, 0, None)]
            gram = np.einsum("rid,rjd->rij", v, v)  # exact integers
            sq = (v * v).sum(-1)
            pd = sq[:, :, None] + sq[:, None, :] - 2 * gram if metric == 1 else -gram
            ties = int(((pd == dist[:, :, None]) & (cand[:, :, None] >= 0) & (cand[:, None, :] >= 0) & (np.arange(K)[None, :, None] > np.arange(K)[None, None, :])).sum())
            assert ties > 0
