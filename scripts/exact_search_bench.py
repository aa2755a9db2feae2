#!/usr/bin/env python
"""lm_exact_search against the stored-table graph search and exact_topk_ip on the benchmark's synthetic corpus (the chunks, encoder and graph
builder of bench.py at its defaults): HIP-event time per call, median of --reps after --warmup, at nq = 1, 16, 256, for an fp32 and an fp16
table.  Every shape that is timed is first compared with the oracle's bruteforce_topk (labels and distance bits; nq <= 16) or with
exact_topk_ip's id sets (nq = 256, where the CPU oracle takes too long).  For nq = 1 the table bytes per second of the exact search are also
given as a fraction of a plain device-to-device copy of the same table measured in the same run.
    python scripts/exact_search_bench.py [--chunks 1000000] [--out profiles/exact_search_1M.json]"""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=1_000_000)
    ap.add_argument("--model", default="sentence-transformers/all-MiniLM-L6-v2")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--ef", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "exact_search_1M.json"))
    args = ap.parse_args()

    import torch

    import bench
    from leann_amd import _lib
    from leann_amd.exact import exact_topk_ip
    from leann_amd.gpu_graph_build import _padded_table, build_graph_gpu
    from leann_amd.index import Mi355xIndex
    from leann_amd.recompute import RecomputeProvider
    from leann_amd.synth import CorpusSpec, SyntheticCorpus
    from leann_amd.token_store import TokenStore
    from oracle import oracle as orc

    _lib.require_gpu()
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    t0 = time.time()
    corpus = SyntheticCorpus(CorpusSpec(n_chunks=args.chunks, seed=1234))
    enc = bench._load_encoder(args.model).to(dev, dtype=torch.float16).eval()
    tok, off = corpus.chunks()
    provider = RecomputeProvider(enc, TokenStore(tok, off, device=0), (enc.cfg.hidden + 63) // 64 * 64, dev)
    X = torch.empty((args.chunks, enc.cfg.hidden), dtype=torch.float32, device=dev)
    for b0 in range(0, args.chunks, 32768):
        ids = torch.arange(b0, min(args.chunks, b0 + 32768), dtype=torch.int32, device=dev)
        X[b0 : b0 + ids.shape[0]] = provider.embed_ids(ids)
    qt, qo, _ = corpus.queries(256, seed=4321)
    Q = RecomputeProvider(enc, TokenStore(qt, qo, device=0), provider.dp, dev).embed_ids(torch.arange(256, dtype=torch.int32, device=dev)).contiguous()
    torch.cuda.synchronize()
    print(f"[exact-bench] corpus of {args.chunks} chunks embedded ({time.time() - t0:.1f}s)", flush=True)
    g = build_graph_gpu(X, "mips", M=32, ef_construction=200) if args.chunks >= 100_000 else build_graph_gpu(X, "mips", M=16, ef_construction=64)
    idx = Mi355xIndex.from_csr(g, device=0)
    idx.set_stream(torch.cuda.current_stream().cuda_stream)
    print(f"[exact-bench] graph built ({time.time() - t0:.1f}s)", flush=True)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return statistics.median(ms)

    k = args.k
    stream = torch.cuda.current_stream().cuda_stream
    Qp = _padded_table(Q)
    res = {"chunks": args.chunks, "d": int(X.shape[1]), "k": k, "ef": args.ef, "reps": args.reps, "warmup": args.warmup, "timing": "HIP events, median", "tables": {}}
    for name, T in (("fp32", _padded_table(X)), ("fp16", _padded_table(X.half()))):
        idx.attach_table(T)
        n, dp = T.shape
        tbytes = T.numel() * T.element_size()
        dst = torch.empty_like(T)
        copy_ms = timed(lambda: dst.copy_(T))
        del dst
        T32_host = None
        rows = {}
        for nq in (1, 16, 256):
            q = Qp[:nq].contiguous()
            D = torch.empty((nq, k), dtype=torch.float32, device=dev)
            L = torch.empty((nq, k), dtype=torch.int64, device=dev)
            nb = int(lib.lm_exact_search_workspace_bytes(n, nq, k))
            ws = torch.empty((max(nb, 8),), dtype=torch.uint8, device=dev)

            def exact():
                _lib.check(lib.lm_exact_search(C.c_void_p(T.data_ptr()), _lib.DTYPE_F16 if T.dtype == torch.float16 else _lib.DTYPE_F32, n, dp, _lib.METRIC_INNER_PRODUCT,
                                               C.c_void_p(q.data_ptr()), nq, k, None, C.c_void_p(D.data_ptr()), C.c_void_p(L.data_ptr()), C.c_void_p(ws.data_ptr()), nb,
                                               C.c_void_p(stream)), "lm_exact_search")

            # correctness first
            exact()
            torch.cuda.synchronize()
            if nq <= 16:
                if T32_host is None:
                    T32_host = T.float().cpu().numpy()
                oi, od = orc.bruteforce_topk(T32_host, q.cpu().numpy(), k, 0)
                checked = "oracle: labels and distance bits equal"
                assert np.array_equal(L.cpu().numpy(), oi) and np.array_equal(D.cpu().numpy().view(np.uint32), od.view(np.uint32)), f"{name} nq={nq}: differs from the oracle"
            else:
                ti = exact_topk_ip(q[:, : X.shape[1]], T[:, : X.shape[1]], k)[1].cpu().numpy()
                li = L.cpu().numpy()
                overlap = float(np.mean([len(set(a.tolist()) & set(b.tolist())) / k for a, b in zip(li, ti)]))
                checked = f"exact_topk_ip id sets: mean overlap {overlap:.4f}"
                assert overlap >= 0.999, f"{name} nq={nq}: id sets differ from exact_topk_ip's ({overlap})"
            prm = idx.make_params(ef=args.ef, beam=1, recompute=False)
            qraw = Q[:nq].contiguous()
            gl = idx.search_device(qraw, k, prm)[1].cpu().numpy()
            recall = float(np.mean([len(set(a.tolist()) & set(b.tolist())) / k for a, b in zip(gl, L.cpu().numpy())]))
            row = {"exact_ms": timed(exact), "graph_ef%d_ms" % args.ef: timed(lambda: idx.search_device(qraw, k, prm)), "graph_recall_at_k_vs_exact": recall,
                   "exact_topk_ip_ms": timed(lambda: exact_topk_ip(q[:, : X.shape[1]], T[:, : X.shape[1]], k)), "checked_against": checked,
                   "slices": int(nb // (nq * k * 8))}
            if nq == 1:
                row["table_bytes"] = tbytes
                row["d2d_copy_ms"] = copy_ms
                row["exact_GBps"] = tbytes / row["exact_ms"] / 1e6
                row["d2d_copy_GBps"] = tbytes / copy_ms / 1e6
                row["exact_fraction_of_copy_rate"] = copy_ms / row["exact_ms"]
            rows[str(nq)] = row
            print(f"[exact-bench] {name} nq={nq}: {json.dumps(row)}", flush=True)
        res["tables"][name] = rows
        del T32_host
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
