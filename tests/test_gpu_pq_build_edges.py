"""lm_pq_encode / lm_pq_train on the MI355X at the shapes tests/emulated_pq_build_cases.py runs on the CPU emulation -- the same lists,
imported from there -- and at those that make every instantiation of k_pq_update (chunk lengths 2, 4, 8, 16, 32 with 256-row tiles; the
run-time length with 128-row tiles and up to 64 coordinates in registers) cross a tile boundary with a ragged tail.  Codes are compared
byte for byte and codebooks bit for bit with the C restatement (tests/pq_ref/lm_pq_ref.c), codes also with argmin over the oracle's
orc_pq_lut; every output is checked for the pre-fill (inside: gone; after the end: untouched).  The premises (centroids that empty
out, repeated centroids of a sample of fewer than 256 rows never winning) are asserted on the restatement's output."""
import numpy as np
import pytest

from tests.emulated_pq_build_cases import ENCODE_SHAPES, TRAIN_SHAPES, _codebooks, _counts, _data, _offsets, _ties_and_nan_inputs, _train_input
from tests.pq_ref_util import lut_argmin_codes, ref_encode, ref_train


def _has_gpu() -> bool:
    try:
        import torch

        return torch.cuda.is_available()
    except Exception:  # noqa: BLE001
        return False


pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not _has_gpu(), reason="needs an MI355X")]


def _uniform(s, length, m, f16, pad=0):
    return (s, length * m, length * m + pad, m, None, f16, "real")


# every k_pq_update instantiation across a tile boundary with a ragged tail: 777 = 3 x 256 + 9 rows for the compiled lengths, 300 =
# 2 x 128 + 44 for the run-time length; fp32 and fp16 each, one of either dtype with ld = d + 64
TILE_TAIL_SHAPES = ([_uniform(777, L, 4, f16, 64 if (L, f16) == (16, True) else 0) for L in (2, 4, 8, 16, 32) for f16 in (False, True)]
                    + [_uniform(300, L, 2 if L == 64 else 4, f16, 64 if (L, f16) == (3, False) else 0) for L in (1, 3, 12, 64) for f16 in (False, True)])
ALL_TRAIN_SHAPES = [(i, sh) for i, sh in enumerate(TRAIN_SHAPES)] + [(100 + i, sh) for i, sh in enumerate(TILE_TAIL_SHAPES)]


def _shape_id(sh):
    s, d, ld, m, off, f16, kind = sh
    return f"s{s}-d{d}-ld{ld}-m{m}-{'chunked' if off is not None else 'uniform'}-{'f16' if f16 else 'f32'}-{kind}"


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    from leann_amd import _lib
    from tests.pq_ref_util import compile_ref, load_ref

    _lib.require_gpu()
    return load_ref(compile_ref(tmp_path_factory.mktemp("pq_ref")))


def test_the_lengths_trained_on_cover_every_instantiation():
    seen = set()
    for _, (s, d, ld, m, off, f16, kind) in ALL_TRAIN_SHAPES:
        if s:
            seen |= set(np.diff(_offsets(d, m, off)).tolist())
    assert {0, 1, 2, 3, 4, 8, 12, 16, 32, 64} <= seen
    for L in (2, 4, 8, 16, 32):  # more than one 256-row tile, and a last one that is not full
        assert any(s > 256 and s % 256 and off is None and d // m == L for _, (s, d, ld, m, off, f16, kind) in ALL_TRAIN_SHAPES)
    for L in (1, 3, 12, 64):     # the run-time length: 128-row tiles
        assert any(s > 128 and s % 128 and off is None and d // m == L for _, (s, d, ld, m, off, f16, kind) in ALL_TRAIN_SHAPES)
    assert any(ld > d and f16 for _, (s, d, ld, m, off, f16, kind) in ALL_TRAIN_SHAPES) and any(ld > d and not f16 for _, (s, d, ld, m, off, f16, kind) in ALL_TRAIN_SHAPES)


@pytest.mark.parametrize("i", range(len(ENCODE_SHAPES)), ids=[f"n{sh[0]}-d{sh[1]}-ld{sh[2]}-m{sh[3]}-{'chunked' if sh[4] is not None else 'uniform'}-{'f16' if sh[5] else 'f32'}-{sh[6]}" for sh in ENCODE_SHAPES])
def test_encode_matches_the_restatement_and_the_lut(ref, i):
    """Every entry of ENCODE_SHAPES (n = 0 and n = 1, m = 1, lengths 0 .. 64, ld > d holding junk that must not be read) with device
    pointers: the restatement's codes and the oracle table's argmin, byte for byte; every code written, nothing after them."""
    from leann_amd import _lib
    from tests.gpu_abi_util import FILL_BYTE, pq_encode

    n, d, ld, m, off, f16, kind = ENCODE_SHAPES[i]
    x = _data(n, d, ld, 300 + i, kind, f16)
    cb = _codebooks(x, d, m, off, 400 + i)
    if ld > d:
        assert (x[:, d:] == 7.5).all()
    rc, got, guard = pq_encode(x, d, cb, off)
    assert rc == _lib.LM_OK
    exp = ref_encode(ref, x, d, cb, off)
    pin = lut_argmin_codes(x, d, cb, off)
    assert np.array_equal(exp, pin)  # (the two references agree: asserted apart, so that a failure below is the kernel's)
    assert got.shape == (n, m) and (guard == FILL_BYTE).all()
    assert np.array_equal(got, exp) and np.array_equal(got, pin)
    rc, again, _ = pq_encode(x, d, cb, off)
    assert rc == _lib.LM_OK and again.tobytes() == got.tobytes()
    if n:  # empty chunks get code 0; duplicates (200.. copy 10..65) never win -- hence no 0xEE = 238 is left either
        assert not bool(got[:, np.diff(_offsets(d, m, off)) == 0].any()) and int(got.max()) < 200


def test_encode_shapes_cover_every_length():
    seen = set()
    for (n, d, ld, m, off, f16, kind) in ENCODE_SHAPES:
        seen |= set(np.diff(_offsets(d, m, off)).tolist())
    assert {0, 1, 2, 3, 4, 8, 12, 16, 32, 64} <= seen


def test_encode_ties_and_nan(ref):
    """case_encode_ties_and_nan's four configurations: ties go to the lowest index, a NaN coordinate of a row makes that chunk's code 0,
    a NaN centroid never wins, +inf distances never win."""
    from leann_amd import _lib
    from tests.gpu_abi_util import FILL_BYTE, pq_encode

    count = 0
    for f16, d, m, off, x, cb, j0, j1 in _ties_and_nan_inputs():
        rc, got, guard = pq_encode(x, d, cb, off)
        assert rc == _lib.LM_OK and (guard == FILL_BYTE).all()
        exp = ref_encode(ref, x, d, cb, off)
        pin = lut_argmin_codes(x, d, cb, off)
        assert np.array_equal(got, exp) and np.array_equal(got, pin), (f16, d, m)
        assert int(got[:, j0].max()) < 7 and got[5, j0] == 0 and got[7, j1] == 3 and got[8, j1] == 0, (f16, d, m)
        count += 1
    assert count == 4


@pytest.mark.parametrize("k", range(len(ALL_TRAIN_SHAPES)), ids=[_shape_id(sh) for _, sh in ALL_TRAIN_SHAPES])
def test_train_matches_the_restatement_bit_for_bit(ref, k):
    """iters 0 / 1 / 5 on every shape of the emulated case's list and of TILE_TAIL_SHAPES; iters = 0 leaves the input bytes untouched; a
    second run returns the same bytes; nothing is written after the codebooks or after the workspace."""
    from leann_amd import _lib
    from tests.gpu_abi_util import FILL_BYTE, FILL_F32_BITS, pq_train

    i, (s, d, ld, m, off, f16, kind) = ALL_TRAIN_SHAPES[k]
    x, init = _train_input(i, s, d, ld, m, off, f16, kind)
    for iters in (0, 1, 5):
        rc, got, cb_guard, ws_guard = pq_train(x, d, init, iters, off)
        assert rc == _lib.LM_OK
        assert (cb_guard == FILL_F32_BITS).all() and (ws_guard == FILL_BYTE).all(), iters
        exp = ref_train(ref, x, d, init, iters, off)
        diff = int((got.view(np.uint32) != exp.view(np.uint32)).sum())
        assert diff == 0, (iters, diff, got.size)
        if iters == 0:
            assert got.tobytes() == np.ascontiguousarray(init, np.float32).tobytes()
        if iters == 5 and s:
            rc, again, _, _ = pq_train(x, d, init, iters, off)
            assert rc == _lib.LM_OK and again.tobytes() == got.tobytes()
            if s > 256:  # (more rows than centroids: the training moved something)
                assert exp.tobytes() != np.ascontiguousarray(init, np.float32).tobytes()


def train_premises(ref):
    """On the restatement alone, over the emulated case's list: centroids that held rows after the first assignment and hold none four
    iterations later; with fewer than 256 rows the repeated centroids never win."""
    emptied = small = 0
    for i, (s, d, ld, m, off, f16, kind) in ALL_TRAIN_SHAPES:
        if not s:
            continue
        x, init = _train_input(i, s, d, ld, m, off, f16, kind)
        c0 = _counts(ref_encode(ref, x, d, init, off))
        c4 = _counts(ref_encode(ref, x, d, ref_train(ref, x, d, init, 4, off), off))
        nz = np.diff(_offsets(d, m, off)) > 0
        if i < 100:
            emptied += int(((c0 > 0) & (c4 == 0))[nz].sum())
        if s < 256:
            small += 1
            assert int((c0[nz][:, s:] > 0).sum()) == 0  # the repeated centroids never win
    return emptied, small


def test_train_premises_hold_on_the_restatement(ref):
    emptied, small = train_premises(ref)
    print(f"centroids that emptied out mid-run: {emptied}; shapes with s < 256: {small}")
    assert emptied > 0 and small > 0


def test_argument_checking_with_device_buffers(ref):
    """tests.emulated_pq_build_cases.argument_envelope -- the emulated case's own list of rejected calls -- against the real library with
    device buffers: every one returns LM_EINVAL and leaves the pre-filled codes, workspace and codebooks as they were."""
    from tests.emulated_pq_build_cases import argument_envelope
    from tests.gpu_abi_util import DevBuf

    argument_envelope(DevBuf, ref)
