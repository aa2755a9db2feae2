"""lm_exact_search helpers shared by tests/emulated_exact_cases.py (host build of the library, numpy buffers) and tests/test_gpu_exact_search.py
(device buffers): test data, the expected result from the oracle -- bruteforce_topk, on the compacted sub-table when there is an allow-list --,
the slicing policy restated from include/leann_mi355x.h, and the entry point called on GUARD-filled output buffers (tests/gpu_abi_util.py's
convention: every output is GUARD elements longer than the kernel owns and pre-filled, so a test can assert that every owned element was written
and nothing after it, the workspace included)."""
from __future__ import annotations

import numpy as np

from tests.gpu_abi_util import FILL_BYTE, FILL_I64, GUARD

WIDTHS = (64, 128, 192, 256, 320, 384, 512, 768, 1024)  # every padded width the kernels cover
QTILE = 8  # queries per tile (csrc/lm_exact_impl.h: EXACT_QT)


def plan(ntable: int, nq: int):
    """(slices, rows per slice): the slicing policy of the header comment, restated."""
    nqt = max(1, -(-nq // QTILE))
    s0 = min(max(1, 512 // nqt), max(1, -(-ntable // 1024)))
    rows = max(32, -(-(-(-ntable // s0)) // 32) * 32)
    return max(1, -(-ntable // rows)), rows


def pad64(x: np.ndarray) -> np.ndarray:
    d = x.shape[1]
    dp = (d + 63) // 64 * 64
    if dp == d:
        return np.ascontiguousarray(x)
    out = np.zeros((x.shape[0], dp), x.dtype)
    out[:, :d] = x
    return out


def gauss_case(n: int, d: int, nq: int, seed: int, f16: bool):
    """Padded (table, queries): normal rows, the second half of the table a copy of the first (exact ties between far-apart ids)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((max(n, 1), d)).astype(np.float32)[:n]
    if n >= 2:
        x[n - n // 2 :] = x[: n // 2]
    q = rng.standard_normal((nq, d)).astype(np.float32)
    return pad64(x.astype(np.float16) if f16 else x), pad64(q)


def integer_case(n: int, d: int, nq: int, seed: int, f16: bool, distinct: int | None = None):
    """Padded (table, queries) with small integer entries (exact in fp16, every distance an exact integer): only `distinct` (default n / 4)
    different vectors, dealt out at random, so equal distances are everywhere -- across slices and around the k-th rank."""
    rng = np.random.default_rng(seed)
    distinct = max(1, n // 4) if distinct is None else distinct
    pool = rng.integers(-3, 4, (distinct, d)).astype(np.float32)
    x = pool[rng.integers(0, distinct, n)]
    q = rng.integers(-3, 4, (nq, d)).astype(np.float32)
    return pad64(x.astype(np.float16) if f16 else x), pad64(q)


def bitmap(mask: np.ndarray, stray_ones: bool = False) -> np.ndarray:
    """bool [ntable] -> uint32 words; stray_ones sets the unused high bits of the last word."""
    n = mask.shape[0]
    bits = np.zeros((n + 31) // 32 * 32, np.uint8)
    bits[:n] = mask
    if stray_ones:
        bits[n:] = 1
    return np.ascontiguousarray(np.packbits(bits, bitorder="little").view("<u4")).astype(np.uint32)


def expected(table: np.ndarray, q: np.ndarray, k: int, metric: int, mask: np.ndarray | None = None):
    """(labels int64 [nq, k], distances fp32 [nq, k]) from oracle.bruteforce_topk; with a mask: on the compacted table of the allowed rows, ids mapped
    back through the sorted allowed-id list (a monotone map: the lower-id tie-break carries over)."""
    from oracle import oracle as orc

    t32 = np.ascontiguousarray(table.astype(np.float32))
    if mask is None:
        ids, dd = orc.bruteforce_topk(t32, q, k, metric)
        return ids, dd
    allowed = np.flatnonzero(mask).astype(np.int64)
    if len(allowed) == 0:  # orc_bruteforce_topk over no rows: every slot empty
        return np.full((q.shape[0], k), -1, np.int64), np.full((q.shape[0], k), np.inf if metric == 1 else -np.inf, np.float32)
    ids, dd = orc.bruteforce_topk(np.ascontiguousarray(t32[allowed]), q, k, metric)
    return np.where(ids >= 0, allowed[np.clip(ids, 0, None)], -1).astype(np.int64), dd


def same(got_l, got_d, exp_l, exp_d) -> bool:
    """labels equal and distance BITS equal"""
    return bool(np.array_equal(got_l, exp_l) and np.array_equal(np.ascontiguousarray(got_d).view(np.uint32), np.ascontiguousarray(exp_d).view(np.uint32)))


def exact_host(lib, table, q, k, metric, words=None, d_padded=None, ntable=None, nq=None, ws_short=0, dtype=None):
    """lm_exact_search on numpy buffers (the emulated library: 'device' pointers are host pointers) -> (rc, labels, distances, untouched) where
    untouched says that the guards after the three buffers -- and, when rc != 0, the buffers themselves -- still hold their fill."""
    n = table.shape[0] if ntable is None else ntable
    b = q.shape[0] if nq is None else nq
    nb = int(lib.lm_exact_search_workspace_bytes(max(n, 0), max(b, 0), k)) if 1 <= k <= 256 else 0
    own = max(b, 0) * max(k, 0)
    D = np.full(own + GUARD, np.nan, np.float32)
    L = np.full(own + GUARD, FILL_I64, np.int64)
    ws = np.full(nb + GUARD, FILL_BYTE, np.uint8)
    rc = lib.lm_exact_search(table.ctypes.data, (1 if table.dtype == np.float16 else 0) if dtype is None else dtype, n, table.shape[1] if d_padded is None else d_padded,
                             metric, q.ctypes.data, b, k, None if words is None else words.ctypes.data, D.ctypes.data, L.ctypes.data, ws.ctypes.data,
                             max(nb - ws_short, 0), None)
    guards = bool(np.isnan(D[own:]).all() and (L[own:] == FILL_I64).all() and (ws[nb:] == FILL_BYTE).all())
    if rc != 0:
        guards = guards and bool(np.isnan(D).all() and (L == FILL_I64).all() and (ws == FILL_BYTE).all())
    return rc, L[:own].reshape(max(b, 0), max(k, 0)), D[:own].reshape(max(b, 0), max(k, 0)), guards


def exact_gpu(table, q, k, metric, words=None):
    """lm_exact_search on device buffers, current stream -> (rc, labels, distances, untouched): as exact_host, and the owned elements are checked
    to be all written (no fill value left: a distance is never NaN -- the key decodes NaN to inf -- and a label never the fill pattern)."""
    import torch

    from leann_amd import _lib

    lib = _lib.load()
    n, b = table.shape[0], q.shape[0]
    nb = int(lib.lm_exact_search_workspace_bytes(n, b, k))
    own = b * k
    tt = torch.from_numpy(np.ascontiguousarray(table)).cuda() if n else torch.zeros((1, table.shape[1]), dtype=torch.float16 if table.dtype == np.float16 else torch.float32, device="cuda")
    tq = torch.from_numpy(np.ascontiguousarray(q)).cuda()
    tw = None if words is None else torch.from_numpy(words.view(np.int32)).cuda()
    D = torch.full((own + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    L = torch.full((own + GUARD,), int(FILL_I64), dtype=torch.int64, device="cuda")
    ws = torch.full((nb + GUARD,), FILL_BYTE, dtype=torch.uint8, device="cuda")
    rc = lib.lm_exact_search(tt.data_ptr(), 1 if table.dtype == np.float16 else 0, n, table.shape[1], metric, tq.data_ptr(), b, k,
                             None if tw is None or tw.numel() == 0 else tw.data_ptr(), D.data_ptr(), L.data_ptr(), ws.data_ptr(), nb, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    hD, hL, hws = D.cpu().numpy(), L.cpu().numpy(), ws.cpu().numpy()
    ok = bool(np.isnan(hD[own:]).all() and (hL[own:] == FILL_I64).all() and (hws[nb:] == FILL_BYTE).all())
    ok = ok and not bool(np.isnan(hD[:own]).any()) and not bool((hL[:own] == FILL_I64).any())
    return rc, hL[:own].reshape(b, k), hD[:own].reshape(b, k), ok
