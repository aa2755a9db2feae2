"""lm_pq_scan / lm_pq_flat_search helpers shared by tests/emulated_pq_flat_cases.py's two worlds (the host build of the library on numpy
buffers, the MI355X on device buffers): the slicing plan restated from include/leann_mi355x.h, test data, and the reference COMPOSED from what
the oracle exports --
    lookup table   oracle.pq_lut_adc (orc_pq_lut);
    ADC            (p0 + p1) + (p2 + p3), p_r the sequential fp32 sum over j = r, r + 4, ... of LUT[j][code[j]] -- restated in numpy over all rows at
                   once and checked against orc_pq_adc on a sample of rows in every call;
    ranking        the (distance, id) key restated: NaN -> +inf, -0 -> +0, lower id first; with an allow-list the allowed rows only;
    rerank         oracle.dist (orc_dist) of every list entry, ranked by the same key.
Labels are compared for equality, distances bit for bit.  The entry point is called on GUARD-filled buffers (tests/gpu_abi_util.py's
convention), the workspace included."""
from __future__ import annotations

import numpy as np

from tests.gpu_abi_util import FILL_BYTE, FILL_I64, GUARD

IP, L2 = 0, 1
MAX_L = 1024        # LM_PQ_FLAT_MAX_L
PQF_CAP = 1280      # csrc/lm_pq_flat_impl.h: pending keys per query
PQF_LDS = 158 * 1024


def plan(ntotal: int, nq: int, m: int, L: int):
    """(queries per tile, slices, rows per slice): the slicing policy of the header comment, restated."""
    per_q = 1024 * m + 16 * L + 8 * PQF_CAP
    qt = min(8, PQF_LDS // per_q)
    nqt = max(1, -(-nq // qt)) if qt > 0 else 1
    s0 = min(max(1, 512 // nqt), max(1, -(-ntotal // 2048)))
    rows = max(32, -(-(-(-ntotal // s0)) // 32) * 32)
    return qt, max(1, -(-ntotal // rows)), rows


def bitmap(mask: np.ndarray, stray_ones: bool = False) -> np.ndarray:
    from tests.gpu_exact_util import bitmap as bm

    return bm(mask, stray_ones)


def offsets(m: int, d: int, lens=None) -> np.ndarray:
    lens = [d // m] * m if lens is None else lens
    assert len(lens) == m and sum(lens) <= d
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def random_pq(n: int, d: int, m: int, seed: int, lens=None):
    """(codebooks, codes, chunk offsets or None): normal centroids -- [m, 256, d / m], or the flat chunked layout for `lens` -- and uniform
    random code bytes (the scan ranks whatever the codes say)."""
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 256, (max(n, 1), m), dtype=np.uint8)[:n]
    if lens is None:
        return rng.standard_normal((m, 256, d // m)).astype(np.float32), codes, None
    off = offsets(m, d, lens)
    return rng.standard_normal(256 * int(off[-1])).astype(np.float32), codes, off


def adc_all(lut: np.ndarray, codes: np.ndarray) -> np.ndarray:
    """orc_pq_adc of every row, in its order, in fp32."""
    n, m = codes.shape
    p = [np.zeros(n, np.float32) for _ in range(4)]
    for j in range(m):
        p[j & 3] = p[j & 3] + lut[j][codes[:, j]]
    return (p[0] + p[1]) + (p[2] + p[3])


def rank(dist: np.ndarray, ids: np.ndarray, L: int, metric: int):
    """The L smallest of the keys (dist, id) -> (labels int64 [L], distances fp32 [L] as the kernels decode them), empty slots -1 / +-inf."""
    with np.errstate(invalid="ignore"):
        d = np.where(np.isnan(dist), np.float32(np.inf), dist).astype(np.float32)
    d = np.where(d == 0, np.float32(0.0), d).astype(np.float32)
    order = np.lexsort((ids, d))[:L]
    lab = np.full(L, -1, np.int64)
    out = np.full(L, np.inf, np.float32)
    lab[: len(order)] = ids[order]
    out[: len(order)] = d[order]
    return lab, (out if metric == L2 else -out)


def expected_scan(cb, codes, q, L: int, metric: int, mask=None, off=None, sample: int = 48):
    """(labels [nq, L], distances [nq, L]) of the flat scan; q: [nq, >= d] fp32."""
    from oracle import oracle as orc

    n = codes.shape[0]
    ids = np.arange(n, dtype=np.int64) if mask is None else np.flatnonzero(mask).astype(np.int64)
    labs, dists = [], []
    for qi in range(q.shape[0]):
        pick = ids[:: max(1, len(ids) // sample)][:sample]
        if n == 0:
            labs.append(np.full(L, -1, np.int64))
            dists.append(np.full(L, np.inf if metric == L2 else -np.inf, np.float32))
            continue
        lut, ref = orc.pq_lut_adc(cb, codes, np.ascontiguousarray(q[qi]), metric, pick, chunk_off=off)
        adc = adc_all(lut, codes[ids])
        mine = adc_all(lut, codes[pick])
        assert np.array_equal(mine.view(np.uint32), ref.view(np.uint32))  # the numpy restatement IS orc_pq_adc
        lab, dd = rank(adc, ids, L, metric)
        labs.append(lab)
        dists.append(dd)
    return np.stack(labs) if labs else np.zeros((0, L), np.int64), np.stack(dists) if dists else np.zeros((0, L), np.float32)


def expected_search(cb, codes, x, q, k: int, L: int, metric: int, mask=None, off=None, rerank: bool = True, table=None):
    """The index form: scan lists of L = max(L, k), exact rerank by orc_dist over `table` (default x; pass the fp16 values widened for an fp16
    table), best k -> (labels [nq, k], distances [nq, k], sorted unique union of the lists)."""
    from oracle import oracle as orc

    L = max(L, k)
    sl, sd = expected_scan(cb, codes, q, L, metric, mask, off)
    union = np.unique(sl[sl >= 0]).astype(np.int32)
    if not rerank:
        return sl[:, :k], sd[:, :k], union
    tab = x if table is None else table
    labs, dists = [], []
    for qi in range(q.shape[0]):
        ids = sl[qi][sl[qi] >= 0]
        dd = np.array([orc.dist(tab[i], q[qi], metric) for i in ids], np.float32)
        lab, out = rank(dd, ids, k, metric)
        labs.append(lab)
        dists.append(out)
    return np.stack(labs), np.stack(dists), union


def same(got_l, got_d, exp_l, exp_d) -> bool:
    """labels equal and distance BITS equal"""
    return bool(np.array_equal(got_l, exp_l) and np.array_equal(np.ascontiguousarray(got_d, dtype=np.float32).view(np.uint32),
                                                                np.ascontiguousarray(exp_d, dtype=np.float32).view(np.uint32)))


class _HostMem:
    """numpy buffers: the emulated library's 'device' pointers are host pointers"""

    def put(self, a):
        a = np.ascontiguousarray(a)
        return a, a.ctypes.data

    def full(self, n, value, dtype):
        a = np.full(n, value, dtype)
        return a, a.ctypes.data

    def get(self, h):
        return h

    stream = None


class _GpuMem:
    def put(self, a):
        import torch

        a = np.ascontiguousarray(a)
        t = torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()
        return t, (t.data_ptr() if t.numel() else None)

    def full(self, n, value, dtype):
        import torch

        tt = {np.float32: torch.float32, np.int64: torch.int64, np.uint8: torch.uint8}[dtype]
        t = torch.full((n,), float(value) if dtype is np.float32 else int(value), dtype=tt, device="cuda")
        return t, t.data_ptr()

    def get(self, h):
        import torch

        torch.cuda.synchronize()
        return h.cpu().numpy()

    @property
    def stream(self):
        import torch

        return torch.cuda.current_stream().cuda_stream


def mem(be):
    return _HostMem() if be.emulated else _GpuMem()


def scan(be, cb, codes, q, L: int, metric: int, words=None, off=None, d=None, ldq=None, ntotal=None, nq=None, m=None, ws_short=0, null=(),
         misalign: int = 0):
    """lm_pq_scan -> (rc, labels [nq, L], distances [nq, L], untouched): untouched says that the guards after the three buffers -- and, when
    rc != 0, the buffers themselves -- still hold their fill; when rc == 0 and rows were scanned, also that every owned output element was written.
    q: [nq, ldq] fp32 (ldq defaults to its width, d to the codebooks' dimension).  `null`: argument names passed as NULL.  misalign: the code
    array starts that many bytes into its allocation."""
    from leann_amd import _lib

    lib = _lib.load()
    M = mem(be)
    mm = codes.shape[1] if m is None else m
    n = codes.shape[0] if ntotal is None else ntotal
    b = q.shape[0] if nq is None else nq
    dd = (int(off[-1]) if off is not None else cb.shape[0] * cb.shape[2]) if d is None else d
    lq = q.shape[1] if ldq is None else ldq
    ok_args = 1 <= L <= MAX_L and mm >= 1 and mm % 4 == 0 and n >= 0 and b >= 0
    nb = int(lib.lm_pq_scan_workspace_bytes(n, b, mm, L)) if ok_args else 0
    own = max(b, 0) * max(L, 0)
    flat = np.zeros(codes.size + misalign, np.uint8)
    flat[misalign:] = codes.reshape(-1)
    hc, pc = M.put(flat)
    hcb, pcb = M.put(np.asarray(cb, np.float32).reshape(-1))
    hq, pq = M.put(np.asarray(q, np.float32))
    hw, pw = (None, None) if words is None else M.put(words)
    D, pD = M.full(own + GUARD, np.nan, np.float32)
    Lb, pL = M.full(own + GUARD, FILL_I64, np.int64)
    ws, pws = M.full(nb + GUARD, FILL_BYTE, np.uint8)
    offh = None if off is None else np.ascontiguousarray(off, np.int32)  # chunk_offsets is a host array
    ptr = dict(codes=None if pc is None else pc + misalign, cb=pcb, q=pq, D=pD, L=pL, ws=pws)
    for name in null:
        ptr[name] = None
    rc = lib.lm_pq_scan(ptr["codes"], n, mm, None if offh is None else offh.ctypes.data, ptr["cb"], dd, metric, ptr["q"], b, lq, L, pw, ptr["D"], ptr["L"],
                        ptr["ws"], max(nb - ws_short, 0), M.stream)
    hD, hL, hws = M.get(D), M.get(Lb), M.get(ws)
    ok = bool(np.isnan(hD[own:]).all() and (hL[own:] == FILL_I64).all() and (hws[nb:] == FILL_BYTE).all())
    if rc != 0:
        ok = ok and bool(np.isnan(hD).all() and (hL == FILL_I64).all() and (hws == FILL_BYTE).all())
    elif b > 0:
        ok = ok and not bool(np.isnan(hD[:own]).any()) and not bool((hL[:own] == FILL_I64).any())  # a decoded key is never NaN
    return rc, hL[:own].reshape(max(b, 0), max(L, 0)).copy(), hD[:own].reshape(max(b, 0), max(L, 0)).copy(), ok
