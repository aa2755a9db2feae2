"""Product quantiser for the DiskANN-style path (index build time) + flat-graph helper.

DiskANN keeps PQ-compressed vectors in memory and traverses on PQ distances
(diskann_backend.py:444-449; compression budget `search_memory_maximum` ~ N*D*4/10 bytes,
:105-111 -> m ~ D*4/10 bytes per vector).  Training (k-means per sub-space) and encoding are
torch ops (any device); the traversal kernel lives in csrc/lm_pq_impl.h.  ``train_pq_kernel`` / ``encode_pq_kernel`` are the same
two steps on the library's kernels (lm_pq_train / lm_pq_encode, csrc/lm_pq_build_impl.h): opt-in, fully specified arithmetic.
"""

from __future__ import annotations

import numpy as np
import torch

from .csr_format import HnswCsr


@torch.no_grad()
def train_pq(x: torch.Tensor, m: int, iters: int = 12, sample: int = 131072, seed: int = 0) -> torch.Tensor:
    """k-means (256 centroids) in each of the m sub-spaces.  Returns codebooks [m, 256, d/m] float32."""
    n, d = x.shape
    if d % m:
        raise ValueError("m must divide d")
    g = torch.Generator(device="cpu").manual_seed(seed)
    idx = torch.randperm(n, generator=g)[: min(n, sample)].to(x.device)
    xs = x[idx].float().view(-1, m, d // m).transpose(0, 1).contiguous()  # [m, s, dsub]
    s = xs.shape[1]
    init = torch.randperm(s, generator=g)[:256].to(x.device)
    if s < 256:
        init = torch.arange(256, device=x.device) % s
    cb = xs[:, init].clone()  # [m, 256, dsub]
    for _ in range(iters):
        d2 = (xs * xs).sum(-1, keepdim=True) - 2 * xs @ cb.transpose(1, 2) + (cb * cb).sum(-1)[:, None, :]
        a = d2.argmin(-1)  # [m, s]
        onehot = torch.zeros((m, s, 256), device=x.device, dtype=xs.dtype)
        onehot.scatter_(2, a.unsqueeze(-1), 1.0)
        cnt = onehot.sum(1)  # [m, 256]
        new = onehot.transpose(1, 2) @ xs  # [m, 256, dsub]
        cb = torch.where(cnt.unsqueeze(-1) > 0, new / cnt.clamp(min=1).unsqueeze(-1), cb)
    return cb.contiguous()


@torch.no_grad()
def encode_pq(x: torch.Tensor, codebooks: torch.Tensor, block: int = 65536) -> torch.Tensor:
    """Nearest centroid per sub-space -> codes [N, m] uint8."""
    n, d = x.shape
    m = codebooks.shape[0]
    out = torch.empty((n, m), dtype=torch.uint8, device=x.device)
    cbn = (codebooks * codebooks).sum(-1)  # [m, 256]
    for b0 in range(0, n, block):
        xs = x[b0 : b0 + block].float().view(-1, m, d // m).transpose(0, 1)  # [m, b, dsub]
        d2 = -2 * xs @ codebooks.transpose(1, 2) + cbn[:, None, :]
        out[b0 : b0 + block] = d2.argmin(-1).transpose(0, 1).to(torch.uint8)
    return out


def _kernel_rows(x: torch.Tensor):
    """x as the library takes it: fp32 or fp16 rows with unit element stride -> (tensor, dtype code, ld, stream)."""
    from . import _lib

    if x.dim() != 2:
        raise ValueError("x must be [N, d]")
    if x.dtype not in (torch.float32, torch.float16):
        x = x.float()
    if x.shape[0] <= 1 or x.shape[1] == 0 or x.stride(1) != 1 or x.stride(0) < x.shape[1]:
        x = x.contiguous()  # (anything but rows of unit element stride at a row stride >= d)
    ld = x.stride(0) if x.shape[0] > 1 and x.shape[1] > 0 else x.shape[1]
    stream = torch.cuda.current_stream(x.device).cuda_stream if x.is_cuda else None
    return x, (_lib.DTYPE_F16 if x.dtype == torch.float16 else _lib.DTYPE_F32), int(ld), stream


def _kernel_chunks(chunk_offsets):
    """chunk_offsets (None = uniform) -> (host int32 array or None, its address or None)."""
    if chunk_offsets is None:
        return None, None
    off = np.ascontiguousarray(np.asarray(chunk_offsets), dtype=np.int32)
    if off.ndim != 1 or off.shape[0] < 2:
        raise ValueError("chunk_offsets must hold m + 1 offsets")
    return off, off.ctypes.data


@torch.no_grad()
def encode_pq_kernel(x: torch.Tensor, codebooks: torch.Tensor, chunk_offsets=None) -> torch.Tensor:
    """encode_pq on the library's kernel (lm_pq_encode) -> codes [N, m] uint8 on x's device.  ``x``: fp32 or fp16 rows, possibly a
    column slice of a wider table (the row stride is passed on).  ``codebooks``: [m, 256, d/m], or -- with ``chunk_offsets`` (m + 1 ints,
    the layout of lm_pq_attach_chunked) -- the flat array of 256 * chunk_offsets[m] floats; columns from chunk_offsets[m] on carry no code.
    The arithmetic is the header's: sequential-fmaf squared L2 as the search's lookup table computes it, ties to the lowest centroid."""
    from . import _lib

    x, dt, ld, stream = _kernel_rows(x)
    n, d = x.shape
    off, off_p = _kernel_chunks(chunk_offsets)
    cb = codebooks.to(device=x.device, dtype=torch.float32).contiguous()
    if off is None:
        if cb.dim() != 3 or cb.shape[1] != 256:
            raise ValueError("codebooks must be [m, 256, d/m]")
        m = int(cb.shape[0])
        if m * cb.shape[2] != d:
            raise ValueError("codebooks [m, 256, dsub] need m * dsub == d")
    else:
        m = int(off.shape[0]) - 1
        if cb.numel() != 256 * max(int(off[-1]), 0):
            raise ValueError("chunked codebooks must hold 256 * chunk_offsets[m] floats")
    codes = torch.empty((n, m), dtype=torch.uint8, device=x.device)
    rc = _lib.load().lm_pq_encode(x.data_ptr(), dt, n, ld, d, m, off_p, cb.data_ptr(), codes.data_ptr(), stream)
    _lib.check(rc, "lm_pq_encode")
    return codes


@torch.no_grad()
def lloyd_kernel(xs: torch.Tensor, codebooks: torch.Tensor, iters: int, chunk_offsets=None) -> torch.Tensor:
    """``iters`` Lloyd iterations (lm_pq_train) over the rows ``xs`` from the centroids ``codebooks`` (layouts as encode_pq_kernel);
    returns the trained codebooks as a new tensor of the same shape."""
    from . import _lib

    xs, dt, ld, stream = _kernel_rows(xs)
    s, d = xs.shape
    off, off_p = _kernel_chunks(chunk_offsets)
    cb = codebooks.to(device=xs.device, dtype=torch.float32).contiguous().clone()
    m = int(cb.shape[0]) if off is None else int(off.shape[0]) - 1
    if off is None and (cb.dim() != 3 or cb.shape[1] != 256 or m * cb.shape[2] != d):
        raise ValueError("codebooks must be [m, 256, d/m]")
    if off is not None and cb.numel() != 256 * max(int(off[-1]), 0):
        raise ValueError("chunked codebooks must hold 256 * chunk_offsets[m] floats")
    lib = _lib.load()
    nbytes = int(lib.lm_pq_train_workspace_bytes(s, d, m))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=xs.device)
    rc = lib.lm_pq_train(xs.data_ptr(), dt, s, ld, d, m, off_p, int(iters), cb.data_ptr(), ws.data_ptr(), nbytes, stream)
    _lib.check(rc, "lm_pq_train")
    return cb


@torch.no_grad()
def train_pq_kernel(x: torch.Tensor, m: int, iters: int = 12, sample: int = 131072, seed: int = 0) -> torch.Tensor:
    """train_pq on the library's kernels (lm_pq_train): the sample and the 256 initial rows are drawn with exactly train_pq's generator
    calls, so both forms start from the same centroids; the iterations then run with the header's arithmetic (sums in ascending row
    order, no atomics: the result is a function of the input bits).  Returns codebooks [m, 256, d/m] float32 on x's device."""
    n, d = x.shape
    if m < 1 or d % m:
        raise ValueError("m must divide d")
    g = torch.Generator(device="cpu").manual_seed(seed)
    idx = torch.randperm(n, generator=g)[: min(n, sample)].to(x.device)
    xs = x[idx]
    if xs.dtype not in (torch.float32, torch.float16):
        xs = xs.float()
    s = xs.shape[0]
    init = torch.randperm(s, generator=g)[:256].to(x.device)
    if s < 256:
        init = torch.arange(256, device=x.device) % max(s, 1)
    if s == 0:
        return torch.zeros((m, 256, d // m), dtype=torch.float32, device=x.device)
    cb = xs[init].float().view(256, m, d // m).transpose(0, 1).contiguous()  # [m, 256, dsub]
    return lloyd_kernel(xs, cb, iters)


@torch.no_grad()
def pq_scan_kernel(codes: torch.Tensor, codebooks: torch.Tensor, queries: torch.Tensor, L: int, metric: str = "mips", chunk_offsets=None,
                   allowed=None):
    """The L best rows of ``codes`` [N, m] uint8 by PQ-ADC distance on the library's kernels (lm_pq_scan) -> (distances [nq, L] float32, labels
    [nq, L] int64) on the codes' device: ADC distance ascending (``"l2"``) or its negation descending (``"mips"``), slots without a row -1 / +-inf.
    ``codebooks`` as for encode_pq_kernel; ``queries`` [nq, d] fp32 (a column slice of wider rows passes its row stride on); ``allowed``: None, a
    bool mask [N] / an array of row ids, or a device int32 tensor that already holds the bitmap words."""
    from . import _lib
    from .index import allow_bitmap

    if codes.dim() != 2 or codes.dtype != torch.uint8:
        raise ValueError("codes must be [N, m] uint8")
    codes = codes.contiguous()
    n, m = int(codes.shape[0]), int(codes.shape[1])
    q = queries.to(device=codes.device, dtype=torch.float32)
    if q.dim() != 2:
        raise ValueError("queries must be [nq, d]")
    if q.shape[0] <= 1 or q.shape[1] == 0 or q.stride(1) != 1 or q.stride(0) < q.shape[1]:
        q = q.contiguous()
    nq, d = int(q.shape[0]), int(q.shape[1])
    ldq = int(q.stride(0)) if nq > 1 and d > 0 else d
    off, off_p = _kernel_chunks(chunk_offsets)
    cb = codebooks.to(device=codes.device, dtype=torch.float32).contiguous()
    if off is None and (cb.dim() != 3 or cb.shape[0] != m or cb.shape[1] != 256 or m * cb.shape[2] != d):
        raise ValueError("codebooks must be [m, 256, d/m]")
    if off is not None and (off.shape[0] != m + 1 or cb.numel() != 256 * max(int(off[-1]), 0)):
        raise ValueError("chunked codebooks must hold 256 * chunk_offsets[m] floats and chunk_offsets m + 1 entries")
    words = None
    if allowed is not None:
        if isinstance(allowed, torch.Tensor) and allowed.dtype == torch.int32 and allowed.device == codes.device and allowed.numel() == (n + 31) // 32:
            words = allowed.contiguous()
        else:
            host = allowed.cpu().numpy() if isinstance(allowed, torch.Tensor) else allowed
            words = torch.from_numpy(allow_bitmap(host, n).view(np.int32)).to(codes.device)
    lib = _lib.load()
    nbytes = int(lib.lm_pq_scan_workspace_bytes(n, nq, m, int(L)))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=codes.device)
    dist = torch.empty((nq, max(int(L), 0)), dtype=torch.float32, device=codes.device)
    labels = torch.empty((nq, max(int(L), 0)), dtype=torch.int64, device=codes.device)
    stream = torch.cuda.current_stream(codes.device).cuda_stream if codes.is_cuda else None
    rc = lib.lm_pq_scan(codes.data_ptr(), n, m, off_p, cb.data_ptr(), d, _lib.METRIC_L2 if metric == "l2" else _lib.METRIC_INNER_PRODUCT, q.data_ptr(),
                        nq, ldq, int(L), None if words is None or words.numel() == 0 else words.data_ptr(), dist.data_ptr(), labels.data_ptr(),
                        ws.data_ptr(), nbytes, stream)
    _lib.check(rc, "lm_pq_scan")
    return dist, labels


def flat_graph(g: HnswCsr, x) -> HnswCsr:
    """Single-level (Vamana-style) graph from the level-0 lists of ``g``, entered at the medoid
    (the node closest to the mean; DiskANN's `<prefix>_disk.index_medoids.bin`).  ``x``: [N, D] numpy array or torch tensor
    (any device; the 10M-chunk configuration passes the HBM-resident table)."""
    n = g.ntotal
    p0 = g.node_offsets[:-1].astype(np.int64)
    beg = g.level_ptr[p0].astype(np.int64)
    end = g.level_ptr[p0 + 1].astype(np.int64)
    deg = end - beg
    level_ptr = np.zeros(2 * n, np.uint64)
    cs = np.cumsum(deg)
    level_ptr[0::2] = cs - deg
    level_ptr[1::2] = cs
    total = int(cs[-1]) if n else 0
    # position of every level-0 entry inside g.neighbors: beg[i] + (k - start[i]) for k in [start[i], start[i] + deg[i])
    idx = np.repeat(beg - (cs - deg), deg) + np.arange(total, dtype=np.int64)
    neighbors = g.neighbors[idx].astype(np.int32)
    medoid = -1
    if n:
        xt = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
        mean = torch.zeros(xt.shape[1], dtype=torch.float64, device=xt.device)
        for b0 in range(0, n, 1 << 20):
            mean += xt[b0 : b0 + (1 << 20)].double().sum(0)
        mean = (mean / n).float()
        best, medoid = float("inf"), 0
        for b0 in range(0, n, 1 << 20):
            d2 = ((xt[b0 : b0 + (1 << 20)].float() - mean) ** 2).sum(1)
            v, i = torch.min(d2, 0)
            if float(v) < best:
                best, medoid = float(v), b0 + int(i)
    return HnswCsr(d=g.d, ntotal=n, metric_type=g.metric_type, levels=np.ones(n, np.int32), level_ptr=level_ptr,
                   node_offsets=np.arange(n + 1, dtype=np.uint64) * 2, neighbors=neighbors, entry_point=medoid,
                   max_level=0 if n else -1, ef_construction=g.ef_construction,
                   cum_nneighbor_per_level=g.cum_nneighbor_per_level)
