"""PQ build scenarios run against libleann_mi355x_emul.so (tests/hip_emul/build_emul_lib.py: the product's kernels on the CPU, a thread
per lane) and the CPU restatement tests/pq_ref/lm_pq_ref.c.  Imported by tests/test_pq_build.py and runnable:
    python -m tests.emulated_pq_build_cases <path/to/libleann_mi355x_emul.so> <path/to/liblm_pq_ref.so> [case ...]
Codes are compared byte for byte, codebooks bit for bit."""
import sys
from pathlib import Path

import numpy as np

CASES = {}
REF = None


def _load(lib_path: str):
    from leann_amd import _lib

    _lib.LIB_PATH = Path(lib_path)
    _lib._lib = None
    return _lib.load()


def _dtype(x):
    from leann_amd import _lib

    return _lib.DTYPE_F16 if x.dtype == np.float16 else _lib.DTYPE_F32


def _m(cb, off):
    return cb.shape[0] if off is None else len(off) - 1


def _kernel_encode(x, d, cb, off=None):
    """lm_pq_encode through the ABI on numpy arrays ('device' pointers are host pointers in the emulated world).  x: [n, ld]."""
    from leann_amd import _lib

    x = np.ascontiguousarray(x)
    cb = np.ascontiguousarray(cb, np.float32)
    o = None if off is None else np.ascontiguousarray(off, np.int32)
    m = _m(cb, off)
    codes = np.full((x.shape[0], m), 0xEE, np.uint8)  # the kernel must write every byte
    rc = _lib.load().lm_pq_encode(x.ctypes.data, _dtype(x), x.shape[0], x.shape[1], d, m, None if o is None else o.ctypes.data, cb.ctypes.data,
                                  codes.ctypes.data, None)
    _lib.check(rc, "lm_pq_encode")
    return codes


def _kernel_train(x, d, init, iters, off=None):
    from leann_amd import _lib

    lib = _lib.load()
    x = np.ascontiguousarray(x)
    cb = np.array(init, np.float32, order="C", copy=True)
    o = None if off is None else np.ascontiguousarray(off, np.int32)
    m = _m(cb, off)
    nb = int(lib.lm_pq_train_workspace_bytes(x.shape[0], d, m))
    ws = np.zeros(max(nb, 1), np.uint8)
    rc = lib.lm_pq_train(x.ctypes.data, _dtype(x), x.shape[0], x.shape[1], d, m, None if o is None else o.ctypes.data, iters, cb.ctypes.data,
                         ws.ctypes.data, nb, None)
    _lib.check(rc, "lm_pq_train")
    return cb


def _offsets(d, m, off):
    return np.arange(m + 1, dtype=np.int64) * (d // m) if off is None else np.asarray(off, np.int64)


def _data(n, d, ld, seed, kind, f16):
    """[n, ld] rows whose first d columns are the vectors; the padding holds junk that must never be read as part of a chunk."""
    rng = np.random.default_rng(seed)
    if kind == "int":
        v = rng.integers(-4, 5, (n, d)).astype(np.float32)
    else:
        cent = rng.standard_normal((12, d)).astype(np.float32)
        v = cent[rng.integers(0, 12, n)] + 0.3 * rng.standard_normal((n, d)).astype(np.float32)
    x = np.full((n, ld), 7.5, np.float32)
    x[:, :d] = v
    return x.astype(np.float16) if f16 else x


def _codebooks(x, d, m, off, seed, dup=True):
    """256 centroids per chunk drawn from the rows (exact zero distances, and -- with fewer than 256 rows or `dup` -- duplicate
    centroids: exact ties).  Uniform: [m, 256, d/m]; chunked: the flat layout."""
    rng = np.random.default_rng(seed)
    o = _offsets(d, m, off)
    n = x.shape[0]
    flat = np.zeros(256 * int(o[-1]), np.float32)
    for j in range(m):
        lo, hi = int(o[j]), int(o[j + 1])
        pick = rng.integers(0, max(n, 1), 256)
        blk = x[pick, lo:hi].astype(np.float32) if n else np.zeros((256, hi - lo), np.float32)
        blk = blk + (rng.random((256, 1)) < 0.5) * rng.standard_normal((256, hi - lo)).astype(np.float32) * 0.1
        if dup:
            blk[200:] = blk[10:66]  # duplicates of earlier centroids: the lower index must win
        flat[256 * lo : 256 * hi] = blk.reshape(-1)
    return flat.reshape(m, 256, d // m) if off is None else flat


ENCODE_SHAPES = [
    # (n, d, ld, m, chunk offsets, fp16, kind)
    (301, 384, 384, 96, None, False, "real"),   # chunk length 4, the 10M configuration's shape
    (1030, 384, 384, 48, None, True, "real"),   # length 8; more rows than one workgroup holds (1024)
    (77, 96, 128, 96, None, False, "real"),     # length 1, rows padded to 64
    (130, 64, 64, 1, None, False, "real"),      # m = 1, length 64 = LM_PQ_MAX_SUB
    (130, 64, 64, 1, None, True, "int"),
    (513, 64, 128, 4, None, True, "real"),      # length 16, padded rows, one row past two 256-row groups
    (257, 64, 64, 2, None, False, "int"),       # length 32
    (1, 48, 48, 24, None, False, "real"),       # n = 1, length 2
    (0, 48, 48, 24, None, False, "real"),       # n = 0
    (100, 60, 64, 20, None, False, "real"),     # length 3
    (99, 60, 60, 5, None, True, "int"),         # length 12
    (211, 130, 130, 8, [0, 3, 3, 10, 11, 27, 27, 59, 123], False, "real"),  # unequal lengths 3 0 7 1 16 0 32 64, 7 trailing dimensions
    (211, 130, 192, 8, [0, 3, 3, 10, 11, 27, 27, 59, 123], True, "real"),
    (150, 40, 64, 9, [0, 4, 8, 12, 20, 28, 28, 32, 32, 32], False, "int"),   # runs of equal lengths, empty chunks at the end too
    (64, 16, 16, 3, [0, 0, 8, 16], True, "int"),                            # an empty first chunk
]


def case_encode_vs_restatement():
    """lm_pq_encode against the restatement and against argmin over the oracle's orc_pq_lut, on every shape of ENCODE_SHAPES."""
    from tests.pq_ref_util import lut_argmin_codes, ref_encode

    seen_len = set()
    for i, (n, d, ld, m, off, f16, kind) in enumerate(ENCODE_SHAPES):
        x = _data(n, d, ld, 300 + i, kind, f16)
        cb = _codebooks(x, d, m, off, 400 + i)
        got = _kernel_encode(x, d, cb, off)
        exp = ref_encode(REF, x, d, cb, off)
        pin = lut_argmin_codes(x, d, cb, off)
        ok = got.shape == (n, m) and np.array_equal(got, exp) and np.array_equal(got, pin)
        if n and i % 3 == 0:  # the same input again: the same bytes
            ok = ok and np.array_equal(_kernel_encode(x, d, cb, off), got)
        o = _offsets(d, m, off)
        seen_len |= set(np.diff(o).tolist())
        if n:  # empty chunks get code 0; duplicates (200.. copy 10..65) never win
            ok = ok and not bool(got[:, np.diff(o) == 0].any()) and int(got.max()) < 200
        print(f"encode n={n} d={d} ld={ld} m={m} chunked={off is not None} f16={f16} {kind}: {'ok' if ok else 'MISMATCH'}", flush=True)
        assert ok
    assert {0, 1, 2, 3, 4, 8, 12, 16, 32, 64} <= seen_len


CASES["encode_vs_restatement"] = case_encode_vs_restatement


def _ties_and_nan_inputs():
    """The four configurations of case_encode_ties_and_nan: (f16, d, m, off, x, cb, j0, j1).  Chunk j0 holds seven distinct centroids, each
    repeated; row 5 has a NaN in chunk j0; centroid 0 of chunk j1 is row 7's chunk with a NaN, centroids 3 and 9 that chunk without it;
    row 8 has +inf in chunk j1."""
    for f16 in (False, True):
        for (d, m, off) in ((32, 8, None), (24, 4, [0, 8, 8, 12, 24])):
            n = 90
            x = _data(n, d, d, 11 + d, "int", f16)
            cb = _codebooks(x, d, m, off, 12 + d, dup=False)
            flat = cb.reshape(-1)
            o = _offsets(d, m, off)
            lens = np.diff(o)
            j0 = int(np.nonzero(lens > 0)[0][0])
            lo, ln = int(o[j0]), int(lens[j0])
            blk = flat[256 * lo : 256 * (lo + ln)].reshape(256, ln)
            blk[:] = blk[np.arange(256) % 7]                  # seven distinct centroids, each repeated: ties everywhere in chunk j0
            x[5, lo] = np.nan                                  # row 5: chunk j0 is all NaN
            j1 = int(np.nonzero(lens > 0)[0][-1])
            lo1, ln1 = int(o[j1]), int(lens[j1])
            blk1 = flat[256 * lo1 : 256 * (lo1 + ln1)].reshape(256, ln1)
            blk1[0] = x[7, lo1 : lo1 + ln1].astype(np.float32)  # centroid 0 of chunk j1 = row 7's chunk exactly ...
            blk1[0, 0] = np.nan                                 # ... but NaN: it must not win
            blk1[3] = x[7, lo1 : lo1 + ln1].astype(np.float32)  # centroid 3 is that chunk without the NaN
            blk1[9] = blk1[3]
            x[8, lo1] = np.inf                                  # row 8: inf - finite = inf in every distance of chunk j1 -> code 0
            yield f16, d, m, off, x, cb, j0, j1


def case_encode_ties_and_nan():
    """Exact ties go to the lowest index; a NaN coordinate in a row makes every distance of that chunk NaN (code 0) and leaves the other
    chunks alone; a NaN coordinate in a centroid removes that centroid only; +inf distances never win against the initial +inf."""
    from tests.pq_ref_util import lut_argmin_codes, ref_encode

    for f16, d, m, off, x, cb, j0, j1 in _ties_and_nan_inputs():
        got = _kernel_encode(x, d, cb, off)
        exp = ref_encode(REF, x, d, cb, off)
        pin = lut_argmin_codes(x, d, cb, off)
        ok = np.array_equal(got, exp) and np.array_equal(got, pin)
        ok = ok and int(got[:, j0].max()) < 7 and got[5, j0] == 0 and got[7, j1] == 3 and got[8, j1] == 0
        print(f"ties/NaN d={d} m={m} chunked={off is not None} f16={f16}: {'ok' if ok else 'MISMATCH'}", flush=True)
        assert ok


CASES["encode_ties_and_nan"] = case_encode_ties_and_nan


def _init_rows(x, d, m, off, rows):
    """Initial centroids = the chunks of the given 256 rows (train_pq's initialisation), in the layout of the codebooks."""
    o = _offsets(d, m, off)
    flat = np.zeros(256 * int(o[-1]), np.float32)
    for j in range(m):
        lo, hi = int(o[j]), int(o[j + 1])
        flat[256 * lo : 256 * hi] = x[rows, lo:hi].astype(np.float32).reshape(-1)
    return flat.reshape(m, 256, d // m) if off is None else flat


def _counts(codes):
    return np.stack([np.bincount(codes[:, j], minlength=256) for j in range(codes.shape[1])])


TRAIN_SHAPES = [
    # (s, d, ld, m, chunk offsets, fp16, kind)
    (700, 32, 32, 8, None, False, "real"),
    (100, 32, 64, 4, None, False, "real"),   # s < 256: init = arange(256) % s
    (700, 32, 32, 16, None, True, "real"),
    (450, 24, 24, 2, None, False, "int"),    # length 12
    (520, 130, 192, 8, [0, 3, 3, 10, 11, 27, 27, 59, 123], False, "real"),
    (300, 130, 130, 8, [0, 3, 3, 10, 11, 27, 27, 59, 123], True, "int"),
    (0, 32, 32, 8, None, False, "real"),
]


def _train_input(i, s, d, ld, m, off, f16, kind):
    """The sample and the initial centroids of train shape number i: 256 of its rows (s < 256: arange(256) % s, train_pq's rule)."""
    x = _data(s, d, ld, 500 + i, kind, f16)
    rng = np.random.default_rng(600 + i)
    rows = (np.arange(256) % s if 0 < s < 256 else rng.permutation(s)[:256]) if s else np.zeros(256, np.int64)
    init = _init_rows(x, d, m, off, rows) if s else np.zeros((m, 256, d // m), np.float32)
    return x, init


def case_train_vs_restatement():
    """lm_pq_train against the restatement, bit for bit: iters 0 / 1 / 5, fewer than 256 rows (repeated centroids that never receive a
    row), clusters that lose all their rows in a later iteration, fp16 input, padded rows, the chunked layout."""
    from tests.pq_ref_util import ref_encode, ref_train

    emptied = 0
    for i, (s, d, ld, m, off, f16, kind) in enumerate(TRAIN_SHAPES):
        x, init = _train_input(i, s, d, ld, m, off, f16, kind)
        for iters in (0, 1, 5):
            got = _kernel_train(x, d, init, iters, off)
            exp = ref_train(REF, x, d, init, iters, off)
            ok = got.tobytes() == exp.tobytes()
            if iters == 0:
                ok = ok and got.tobytes() == np.ascontiguousarray(init, np.float32).tobytes()
            if iters == 5 and s:
                ok = ok and _kernel_train(x, d, init, iters, off).tobytes() == got.tobytes()  # twice: the same bits
            print(f"train s={s} d={d} ld={ld} m={m} chunked={off is not None} f16={f16} {kind} iters={iters}: {'ok' if ok else 'MISMATCH'}", flush=True)
            assert ok
        if s:  # centroids that held rows after the first assignment and hold none later (they keep their last mean)
            c0 = _counts(ref_encode(REF, x, d, init, off))
            c4 = _counts(ref_encode(REF, x, d, ref_train(REF, x, d, init, 4, off), off))
            nz = np.diff(_offsets(d, m, off)) > 0
            emptied += int(((c0 > 0) & (c4 == 0))[nz].sum())
            if s < 256:
                assert int((c0[nz][:, s:] > 0).sum()) == 0  # the repeated centroids never win
    print(f"centroids that emptied out mid-run: {emptied}", flush=True)
    assert emptied > 0


CASES["train_vs_restatement"] = case_train_vs_restatement


def _separated_integer_data(seed):
    """400 points in 200 well-separated pairs: integer coordinates, cluster centres on a grid of step 64, two points per cluster a few
    units apart.  Every sum of a cluster's points is an exact fp32 integer, so both forms compute the same means from the same
    assignment; the assignment itself is checked to be tie-free with a margin (_assert_margin)."""
    rng = np.random.default_rng(seed)
    d = 64  # (sub-spaces of >= 8 dimensions: 7^8 grid points, so two clusters do not share a centre inside a chunk)
    cent = rng.integers(-3, 4, (200, d)) * 64
    x = np.repeat(cent, 2, axis=0) + rng.integers(-10, 11, (400, d))
    return x[rng.permutation(400)].astype(np.float32)


def _assert_margin(x, cb, dsub):
    """Independent float64 check of the case's premise: for every row and chunk, the gap between the nearest centroid VALUE and the
    second nearest distinct value exceeds twice a bound on the fp32 rounding error of either form of one squared distance ((dsub + 3)
    ulps of |x|^2 + 2 |x.c| + |c|^2, the largest over the row's centroids): one error for each of the two distances compared.  Identical centroids tie exactly in both forms (lowest index wins in both)."""
    m = cb.shape[0]
    worst = np.inf
    for j in range(m):
        xs = x[:, j * dsub : (j + 1) * dsub].astype(np.float64)
        c = cb[j].astype(np.float64)
        d2 = ((xs[:, None, :] - c[None, :, :]) ** 2).sum(-1)  # [n, 256]
        mag = (xs * xs).sum(-1)[:, None] + 2 * np.abs(xs @ c.T) + (c * c).sum(-1)[None, :]
        err = (dsub + 3) * 2.0 ** -23 * mag.max(1)
        best = d2.min(1)
        same = np.all(c[None, :, :] == c[d2.argmin(1)][:, None, :], axis=-1)  # centroids equal to the winner
        second = np.where(same, np.inf, d2).min(1)
        worst = min(worst, float(((second - best) / (2 * err)).min()))
    assert worst > 1.0, worst
    return worst


def case_agreement_with_the_torch_form():
    """Integer-valued, well-separated data: train_pq_kernel / encode_pq_kernel (on CPU tensors over the emulated library) return the
    codebooks and codes of train_pq / encode_pq, bit for bit."""
    import torch

    from leann_amd.pq import encode_pq, encode_pq_kernel, train_pq, train_pq_kernel
    from tests.pq_ref_util import ref_train

    for seed, m in ((1, 4), (2, 8)):
        xn = _separated_integer_data(seed)
        x = torch.from_numpy(xn)
        d = xn.shape[1]
        iters = 4
        cb_t = train_pq(x, m, iters=iters, seed=seed)
        cb_k = train_pq_kernel(x, m, iters=iters, seed=seed)
        # the premise, checked on the restatement's trajectory from the common start
        g = torch.Generator(device="cpu").manual_seed(seed)
        idx = torch.randperm(400, generator=g)
        init = torch.randperm(400, generator=g)[:256]
        xs = xn[idx.numpy()]
        start = np.ascontiguousarray(xs[init.numpy()].reshape(256, m, d // m).transpose(1, 0, 2))
        margins = [_assert_margin(xs, ref_train(REF, xs, d, start, k), d // m) for k in range(iters)]
        margins.append(_assert_margin(xn, cb_k.numpy(), d // m))
        co_t, co_k = encode_pq(x, cb_t), encode_pq_kernel(x, cb_k)
        ok = cb_k.dtype == torch.float32 and tuple(cb_k.shape) == (m, 256, d // m) and cb_t.numpy().tobytes() == cb_k.numpy().tobytes()
        ok = ok and co_k.dtype == torch.uint8 and np.array_equal(co_t.numpy(), co_k.numpy())
        print(f"torch agreement seed={seed} m={m}: smallest gap {min(margins):.1f} x the two distances' error bound: {'ok' if ok else 'MISMATCH'}", flush=True)
        assert ok


CASES["agreement_with_the_torch_form"] = case_agreement_with_the_torch_form


def case_quality_against_the_torch_form():
    """N(0,1) around 64 centres, 20 000 x 64, m = 16, iters = 8: the reconstruction MSE of the kernel-trained quantiser may exceed that of
    torch's train_pq (same sample, same initial centroids: seed 0) by no more than train_pq's own seed-to-seed spread,
    (max - min) / min over seeds 0..4 -- both are Lloyd descents from one start that part only at near-ties."""
    import torch

    from leann_amd.pq import encode_pq, encode_pq_kernel, train_pq, train_pq_kernel
    from tests.pq_ref_util import recon_mse

    rng = np.random.default_rng(2024)
    cent = 4.0 * rng.standard_normal((64, 64)).astype(np.float32)
    xn = (cent[rng.integers(0, 64, 20000)] + rng.standard_normal((20000, 64)).astype(np.float32)).astype(np.float32)
    x = torch.from_numpy(xn)
    mses = []
    for seed in range(5):
        cb = train_pq(x, 16, iters=8, seed=seed)
        mses.append(recon_mse(xn, cb.numpy(), encode_pq(x, cb).numpy()))
    spread = (max(mses) - min(mses)) / min(mses)
    cbk = train_pq_kernel(x, 16, iters=8, seed=0)
    mk = recon_mse(xn, cbk.numpy(), encode_pq_kernel(x, cbk).numpy())
    print(f"quality: torch MSE by seed {[round(v, 6) for v in mses]}, spread {spread:.6f}; kernel MSE (seed 0) {mk:.6f} = torch seed 0 x {mk / mses[0]:.6f}", flush=True)
    assert mk <= mses[0] * (1.0 + spread), (mk, mses, spread)


CASES["quality_against_the_torch_form"] = case_quality_against_the_torch_form


def case_builder_wiring():
    """Both builders with gpu_pq_kernel=True write a bundle that loads and whose codes are encode_pq_kernel of the written codebooks;
    with the default the arrays in <stem>_pq.npz are those of the untouched train_pq / encode_pq."""
    import inspect
    import tempfile

    import torch

    from leann_amd import backend
    from leann_amd.csr_format import read_index
    from leann_amd.pq import encode_pq, encode_pq_kernel, train_pq, train_pq_kernel
    from tests.util import clustered

    assert inspect.signature(backend._make_pq).parameters["gpu_pq_kernel"].default is False
    backend._pq_kernel_device = lambda: torch.device("cpu")  # the emulated library's device memory is host memory
    calls = {"kernel": 0}
    from leann_amd import pq as pqmod

    real = pqmod.train_pq_kernel

    def counting(*a, **k):
        calls["kernel"] += 1
        return real(*a, **k)

    pqmod.train_pq_kernel = counting
    x = clustered(700, 32, 9, n_centers=16, sigma=0.5)
    xt = torch.from_numpy(x)
    ids = [str(i) for i in range(x.shape[0])]
    with tempfile.TemporaryDirectory() as td:
        for name, make in (("hnsw", lambda **k: backend.Mi355xBuilder(M=8, efConstruction=40, distance_metric="l2", is_recompute=False, is_compact=False, pq_bytes=8, **k)),
                           ("diskann", lambda **k: backend.Mi355xDiskannBuilder(graph_degree=16, complexity=32, distance_metric="l2", pq_bytes=8, **k))):
            pk, pd = Path(td) / f"{name}_k" / "i.index", Path(td) / f"{name}_d" / "i.index"
            before = calls["kernel"]
            make(gpu_pq_kernel=True).build(x, ids, str(pk))
            assert calls["kernel"] == before + 1
            make().build(x, ids, str(pd))
            assert calls["kernel"] == before + 1  # the default never touches the kernels
            zk, zd = np.load(pk.parent / "i_pq.npz"), np.load(pd.parent / "i_pq.npz")
            g = read_index(pk.parent / "i.index")
            ok = g.ntotal == 700 and zk["codebooks"].shape == (8, 256, 4) and zk["codebooks"].dtype == np.float32 and zk["codes"].dtype == np.uint8
            ok = ok and np.array_equal(zk["codes"], encode_pq_kernel(xt, torch.from_numpy(zk["codebooks"])).numpy())
            ok = ok and zk["codebooks"].tobytes() == real(xt, 8, seed=0).numpy().tobytes()
            cb = train_pq(xt, 8, seed=0)
            ok = ok and zd["codebooks"].tobytes() == cb.numpy().tobytes() and zd["codes"].tobytes() == encode_pq(xt, cb).numpy().tobytes()
            print(f"builder wiring {name}: {'ok' if ok else 'MISMATCH'}", flush=True)
            assert ok
    pqmod.train_pq_kernel = real
    assert train_pq_kernel is real


CASES["builder_wiring"] = case_builder_wiring


class _HostBuf:
    """A buffer of the emulated world, where 'device' memory is host memory: .ptr for the ABI, .host() to read it back."""

    def __init__(self, a):
        self.a = a
        self.ptr = a.ctypes.data

    def host(self):
        return self.a


def argument_envelope(buf, ref):
    """The library-level half of case_argument_checking over buffers made by `buf(array)` (an object with .ptr and .host()): host
    memory for the emulated library, device memory on the MI355X (tests/test_gpu_pq_build_edges.py runs this very function)."""
    import pytest

    from leann_amd import _lib

    lib = _lib.load()
    x = buf(np.zeros((8, 16), np.float32))
    cb = buf(np.full((4, 256, 4), 0.25, np.float32))
    good = dict(x=x.ptr, dtype=0, n=8, ld=16, d=16, m=4, off=None, cb=cb.ptr, iters=2)
    offs = {}

    def offp(v):  # chunk_offsets is a host array in both worlds
        if v is None:
            return None
        offs["keep"] = np.ascontiguousarray(v, np.int32)
        return offs["keep"].ctypes.data

    def enc(out, **over):
        a = dict(good, **over)
        return lib.lm_pq_encode(a["x"], a["dtype"], a["n"], a["ld"], a["d"], a["m"], offp(a["off"]), a["cb"], a.get("codes", out.ptr), None)

    def trn(wsp, **over):
        a = dict(good, **over)
        return lib.lm_pq_train(a["x"], a["dtype"], a["n"], a["ld"], a["d"], a["m"], offp(a["off"]), a["iters"], a["cb"], a.get("ws", wsp.ptr),
                               a.get("wsb", wsp.host().nbytes), None)

    shape_bad = [dict(dtype=2), dict(dtype=-1), dict(ld=15), dict(m=0), dict(m=-2), dict(m=4097), dict(m=3), dict(n=-1),
                 dict(off=[1, 4, 8, 12, 16]), dict(off=[0, 8, 4, 12, 16]), dict(off=[0, 4, 8, 12, 17]), dict(x=None), dict(cb=None),
                 dict(m=1, d=80, ld=80),                                  # uniform chunk of 80 > LM_PQ_MAX_SUB
                 dict(m=2, d=80, ld=80, off=[0, 65, 80])]                 # chunked: 65 > LM_PQ_MAX_SUB
    codes = buf(np.full((8, 4), 0xEE, np.uint8))
    need = int(lib.lm_pq_train_workspace_bytes(8, 16, 4))
    assert need >= 8 * 4
    ws = buf(np.full(need, 0xEE, np.uint8))
    cb0 = cb.host().tobytes()
    for over in shape_bad + [dict(codes=None)]:
        with pytest.raises(ValueError):
            _lib.check(enc(codes, **over), "lm_pq_encode")
        assert (codes.host() == 0xEE).all(), over
    for over in shape_bad + [dict(iters=-1), dict(ws=None), dict(wsb=need - 1), dict(wsb=0)]:
        with pytest.raises(ValueError):
            _lib.check(trn(ws, **over), "lm_pq_train")
        assert (ws.host() == 0xEE).all() and cb.host().tobytes() == cb0, over
    assert _lib.last_error()
    # nothing to do: fine, and still nothing written (NULL buffers are allowed when there are no rows)
    _lib.check(enc(codes, n=0, x=None, cb=None, codes=None))
    _lib.check(trn(ws, n=0, x=None, cb=None, ws=None, wsb=0))
    _lib.check(trn(ws, iters=0))
    assert (codes.host() == 0xEE).all() and (ws.host() == 0xEE).all() and cb.host().tobytes() == cb0
    # m % 4 is not required here; a well-formed call writes every code
    cb3 = np.ascontiguousarray(np.random.default_rng(0).standard_normal((3, 256, 4)), np.float32)
    x12 = np.ascontiguousarray(np.random.default_rng(1).standard_normal((8, 12)), np.float32)
    c3 = buf(np.full((8, 3), 0xEE, np.uint8))
    bx12, bcb3 = buf(x12), buf(cb3)
    _lib.check(lib.lm_pq_encode(bx12.ptr, 0, 8, 12, 12, 3, None, bcb3.ptr, c3.ptr, None))
    from tests.pq_ref_util import ref_encode

    assert np.array_equal(c3.host(), ref_encode(ref, x12, 12, cb3))
    _lib.check(enc(codes))
    assert (codes.host() == 0).all()  # every centroid equal: the lowest index


def case_argument_checking():
    """Every argument the header rejects returns LM_EINVAL (ValueError through _lib.check) and launches nothing: the output buffers keep
    their fill.  n == 0 / s == 0 / iters == 0 are fine."""
    import pytest
    import torch

    from leann_amd.pq import encode_pq_kernel, train_pq_kernel

    argument_envelope(_HostBuf, REF)
    print("argument checking: ok", flush=True)
    # the wrappers raise ValueError for the same envelope
    xt = torch.zeros((10, 16))
    with pytest.raises(ValueError):
        encode_pq_kernel(xt, torch.zeros((3, 256, 4)))          # m * dsub != d
    with pytest.raises(ValueError):
        encode_pq_kernel(torch.zeros((10, 80)), torch.zeros((1, 256, 80)))  # chunk longer than LM_PQ_MAX_SUB: the library refuses
    with pytest.raises(ValueError):
        encode_pq_kernel(xt, torch.zeros(256 * 16), chunk_offsets=[0, 8, 4, 16])
    with pytest.raises(ValueError):
        train_pq_kernel(xt, 3)
    with pytest.raises(ValueError):
        train_pq_kernel(xt, 4, iters=-1)
    with pytest.raises(ValueError):
        train_pq_kernel(torch.zeros((10, 130)), 1)
    assert tuple(encode_pq_kernel(torch.zeros((0, 16)), torch.zeros((4, 256, 4))).shape) == (0, 4)
    # a column slice of a wider table is passed with its row stride, not copied: same codes as the contiguous copy
    wide = torch.from_numpy(np.random.default_rng(3).standard_normal((50, 64)).astype(np.float32))
    cbt = torch.from_numpy(np.random.default_rng(4).standard_normal((4, 256, 4)).astype(np.float32))
    assert torch.equal(encode_pq_kernel(wide[:, :16], cbt), encode_pq_kernel(wide[:, :16].contiguous(), cbt))
    print("wrapper checking: ok", flush=True)


CASES["argument_checking"] = case_argument_checking


if __name__ == "__main__":
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    _load(sys.argv[1])
    from tests.pq_ref_util import load_ref

    REF = load_ref(sys.argv[2])
    import time

    import torch

    torch.set_num_threads(1)
    for name in (sys.argv[3:] or list(CASES)):
        t0 = time.time()
        CASES[name]()
        print(f"[case {name}: {time.time() - t0:.1f} s]", flush=True)
    print("ALL CASES OK")
