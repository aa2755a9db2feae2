"""Exact (brute-force) top-k of inner products on the GPU: the ground truth of the benchmarks' recall figures.

Measurement helper -- nothing on the search path uses it.  Written as a blocked loop on purpose: a single ``Q @ X.T`` whose OUTPUT has
more than 2^31 elements comes back wrong from the GEMM library on this stack (round 4, BASELINE configs[2] at 10M chunks: 256 queries x
10M chunks = 2.56e9 scores; rows 215 .. 255 of every 256-query block were garbage, which capped every recall figure of that run at
214.7 / 256 = 0.84 -- for the graph search, for a brute-force ADC ranking and for every candidate-list size alike)."""
from __future__ import annotations

import torch

MAX_SCORES = 1 << 28  # scores per GEMM call: far below 2^31, ~1 GiB of fp32


@torch.no_grad()
def exact_topk_ip(Q: torch.Tensor, X: torch.Tensor, k: int, q_block: int = 256):
    """(values [nq, k] f32, indices [nq, k] i64) of the k largest Q X^T per query, ties broken by torch.topk.  Q [nq, D], X [n, D] fp32."""
    nq, n = Q.shape[0], X.shape[0]
    k = min(k, n)
    x_block = max(k, min(n, MAX_SCORES // max(1, min(q_block, nq))))
    vals = torch.empty((nq, k), dtype=torch.float32, device=Q.device)
    idxs = torch.empty((nq, k), dtype=torch.int64, device=Q.device)
    for b0 in range(0, nq, q_block):
        qb = Q[b0 : b0 + q_block].float()
        bv = bi = None
        for c0 in range(0, n, x_block):
            v, i = torch.topk(qb @ X[c0 : c0 + x_block].float().T, min(k, n - c0), dim=1)
            i = i + c0
            if bv is None:
                bv, bi = v, i
            else:
                cv, ci = torch.cat((bv, v), 1), torch.cat((bi, i), 1)
                sel = torch.topk(cv, k, dim=1).indices
                bv, bi = torch.gather(cv, 1, sel), torch.gather(ci, 1, sel)
        vals[b0 : b0 + qb.shape[0]], idxs[b0 : b0 + qb.shape[0]] = bv, bi
    return vals, idxs


def exact_topk_kernel(Q: torch.Tensor, X: torch.Tensor, k: int, metric: str = "mips"):
    """(values [nq, k] f32, indices [nq, k] i64) shaped like :func:`exact_topk_ip`'s, through lm_exact_search: the canonical distance and the
    (distance, id) order of the oracle's bruteforce_topk, so the result can be compared bit for bit with it.  Q [nq, D] fp32, X [n, D] fp32 or
    fp16, on the same device; both are padded by the table rule of the library (gpu_graph_build._padded_table).  metric "mips" / "cosine" (inner
    product, largest first) or "l2" (squared L2, smallest first).  k <= min(n, LM_EXACT_MAX_K)."""
    import ctypes as C

    from . import _lib
    from .gpu_graph_build import _padded_table

    nq, n = Q.shape[0], X.shape[0]
    k = min(k, n)
    xt, qt = _padded_table(X), _padded_table(Q.float())
    dp = xt.shape[1]
    lib = _lib.load()
    vals = torch.empty((nq, k), dtype=torch.float32, device=Q.device)
    idxs = torch.empty((nq, k), dtype=torch.int64, device=Q.device)
    nbytes = int(lib.lm_exact_search_workspace_bytes(n, nq, k))
    ws = torch.empty((max(nbytes, 8),), dtype=torch.uint8, device=Q.device)
    stream = torch.cuda.current_stream(Q.device).cuda_stream if Q.is_cuda else None
    _lib.check(lib.lm_exact_search(C.c_void_p(xt.data_ptr()), _lib.DTYPE_F16 if xt.dtype == torch.float16 else _lib.DTYPE_F32, n, dp,
                                   _lib.METRIC_L2 if metric.lower() == "l2" else _lib.METRIC_INNER_PRODUCT, C.c_void_p(qt.data_ptr()), nq, k, None,
                                   C.c_void_p(vals.data_ptr()), C.c_void_p(idxs.data_ptr()), C.c_void_p(ws.data_ptr()), nbytes, C.c_void_p(stream)),
               "lm_exact_search")
    if Q.is_cuda:
        torch.cuda.current_stream(Q.device).synchronize()
    return vals, idxs
