"""The stand-alone and build-time entry points of libleann_mi355x.so called through leann_amd._lib with torch device tensors' data_ptr()
on the current stream, for the GPU edge-case modules (tests/test_gpu_select_edges.py, tests/test_gpu_pq_build_edges.py and the
lm_dist_gather / lm_topk_merge cases of tests/test_gpu_parity.py).

Every output buffer is allocated GUARD elements longer than the kernel owns and pre-filled -- 0xEE in every byte, NaN (FILL_F32_BITS) in
every float -- so that a test can assert that the kernel wrote every element it owns and nothing after them, as the emulated helpers
(tests/emulated_select_cases.py, tests/emulated_pq_build_cases.py) do on host memory.  Each call returns the ABI's return code first;
nothing here raises on LM_EINVAL, so the rejected calls are tested through the same functions."""
from __future__ import annotations

import numpy as np

GUARD = 512
FILL_BYTE = 0xEE
FILL_I64 = np.frombuffer(bytes([FILL_BYTE] * 8), np.int64)[0]
FILL_F32_BITS = 0x7FC00000  # torch.full(..., nan)


def _torch():
    import torch

    return torch


def dev(a: np.ndarray):
    """A contiguous device copy of a numpy array."""
    torch = _torch()
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ptr(t):
    return None if t is None or t.numel() == 0 else t.data_ptr()


def _stream():
    return _torch().cuda.current_stream().cuda_stream


def byte_buffer(n: int):
    torch = _torch()
    return torch.full((n + GUARD,), FILL_BYTE, dtype=torch.uint8, device="cuda")


def float_buffer(n: int):
    torch = _torch()
    return torch.full((n + GUARD,), float("nan"), dtype=torch.float32, device="cuda")


def _host(t) -> np.ndarray:
    _torch().cuda.synchronize()
    return t.cpu().numpy()


def _dtype(a: np.ndarray) -> int:
    from leann_amd import _lib

    return _lib.DTYPE_F16 if a.dtype == np.float16 else _lib.DTYPE_F32


class DevBuf:
    """tests.emulated_pq_build_cases.argument_envelope's buffer on the device: .ptr for the ABI, .host() reads it back."""

    def __init__(self, a: np.ndarray):
        self.t = dev(a)
        self.shape = a.shape
        self.ptr = self.t.data_ptr()

    def host(self) -> np.ndarray:
        return _host(self.t).reshape(self.shape)


def select_neighbors(table: np.ndarray, cand: np.ndarray, dist: np.ndarray, m: int, metric: int, alpha: float, d_padded: int | None = None):
    """-> (rc, keep uint8 [n, K], guard uint8 [GUARD]).  table: [ntable, >= d_padded] fp32 / fp16 rows; d_padded defaults to its width."""
    from leann_amd import _lib

    t, c, d = dev(table), dev(cand.astype(np.int32)), dev(dist.astype(np.float32))
    n, K = cand.shape
    keep = byte_buffer(n * K)
    rc = _lib.load().lm_select_neighbors(_ptr(t), _dtype(table), table.shape[0], table.shape[1] if d_padded is None else d_padded, metric, _ptr(c), _ptr(d),
                                         n, K, m, alpha, keep.data_ptr(), _stream())
    h = _host(keep)
    return rc, h[: n * K].reshape(n, K), h[n * K :]


def _offsets_ptr(off, hold):
    if off is None:
        return None
    hold.append(np.ascontiguousarray(off, np.int32))  # chunk_offsets is a host array
    return hold[-1].ctypes.data


def _n_chunks(cb: np.ndarray, off) -> int:
    return cb.shape[0] if off is None else len(off) - 1


def pq_encode(x: np.ndarray, d: int, cb: np.ndarray, off=None):
    """-> (rc, codes uint8 [n, m], guard).  x: [n, ld] fp32 / fp16; cb: [m, 256, d / m] or the flat chunked layout with `off`."""
    from leann_amd import _lib

    hold = []
    m = _n_chunks(cb, off)
    n = x.shape[0]
    tx, tcb = dev(x), dev(cb.astype(np.float32))
    codes = byte_buffer(n * m)
    rc = _lib.load().lm_pq_encode(_ptr(tx), _dtype(x), n, x.shape[1], d, m, _offsets_ptr(off, hold), _ptr(tcb), codes.data_ptr(), _stream())
    h = _host(codes)
    return rc, h[: n * m].reshape(n, m), h[n * m :]


def pq_train(x: np.ndarray, d: int, init: np.ndarray, iters: int, off=None):
    """-> (rc, codebooks fp32 in init's shape, guard after the codebooks as uint32 words, guard after the workspace).  The codebooks
    live in a NaN-filled buffer GUARD floats longer than they are; the workspace is lm_pq_train_workspace_bytes long plus GUARD bytes."""
    from leann_amd import _lib

    lib = _lib.load()
    hold = []
    m = _n_chunks(init, off)
    s = x.shape[0]
    init = np.ascontiguousarray(init, np.float32)
    tx = dev(x)
    cb = float_buffer(init.size)
    cb[: init.size] = dev(init.reshape(-1))
    nb = int(lib.lm_pq_train_workspace_bytes(s, d, m))
    ws = byte_buffer(nb)
    rc = lib.lm_pq_train(_ptr(tx), _dtype(x), s, x.shape[1], d, m, _offsets_ptr(off, hold), iters, cb.data_ptr(), ws.data_ptr(), nb, _stream())
    h = _host(cb)
    return rc, h[: init.size].reshape(init.shape).copy(), h[init.size :].view(np.uint32), _host(ws)[nb:]


def dist_gather(table: np.ndarray, d_padded: int, metric: int, q: np.ndarray, qidx: np.ndarray, ids: np.ndarray):
    """-> (rc, out fp32 [npairs], guard as uint32 words).  table: [n, d_padded] fp32 / fp16; q: fp32 [nq, d_padded]."""
    from leann_amd import _lib

    npairs = ids.shape[0]
    tt, tq, tqi, ti = dev(table), dev(q.astype(np.float32)), dev(qidx.astype(np.int32)), dev(ids.astype(np.int32))
    out = float_buffer(npairs)
    rc = _lib.load().lm_dist_gather(_ptr(tt), _dtype(table), d_padded, metric, _ptr(tq), _ptr(tqi), _ptr(ti), npairs, out.data_ptr(), _stream())
    h = _host(out)
    return rc, h[:npairs], h[npairs:].view(np.uint32)


def topk_merge(ids: np.ndarray, dist: np.ndarray, metric: int):
    """ids int64 / dist fp32 [S, B, k] -> (rc, out_ids int64 [B, k], out_dist fp32 [B, k], id guard int64, dist guard uint32 words)."""
    from leann_amd import _lib

    torch = _torch()
    S, B, k = ids.shape
    ti, td = dev(ids.astype(np.int64)), dev(dist.astype(np.float32))
    oi = byte_buffer(8 * (B * k + GUARD)).view(torch.int64)[: B * k + GUARD]
    od = float_buffer(B * k)
    rc = _lib.load().lm_topk_merge(_ptr(ti), _ptr(td), S, B, k, metric, oi.data_ptr(), od.data_ptr(), _stream())
    hi, hd = _host(oi), _host(od)
    return rc, hi[: B * k].reshape(B, k), hd[: B * k].reshape(B, k), hi[B * k :], hd[B * k :].view(np.uint32)
