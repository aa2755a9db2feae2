#!/usr/bin/env python
"""The flat PQ scan (lm_pq_scan) and the filtered search built on it (lm_pq_flat_search) on the benchmark's synthetic corpus (the chunks,
encoder and graph builder of bench.py at its defaults), m = 96: HIP-event time per call, median of --reps after --warmup.
  scan      lm_pq_scan at 1 / 8 / 64 queries, L = --L: time and code bytes per second;
  filtered  at selectivities 100 % / 10 % / 1 % / 0.1 %, 16 queries: lm_pq_flat_search (rerank through the recompute provider: the pruned index's
            mode) against the recompute graph search followed by a post-filter (time and the mean number of hits that survive the filter), and
            against lm_index_search_exact under the same allow-list on a table-carrying copy of the index;
  recall    recall@k of lm_pq_flat_search against that exact filtered result at L = 64 / 256 / 1024, per selectivity.
Before anything is timed the scan is compared, on the first 20000 rows, with the oracle's lookup table and ADC sum ranked by (distance, id).
    python scripts/pq_flat_bench.py [--chunks 1000000] [--out profiles/pq_flat_1M.json]"""
import argparse
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
    ap.add_argument("--m", type=int, default=96)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--L", type=int, default=64)
    ap.add_argument("--ef", type=int, default=64)
    ap.add_argument("--nq", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "pq_flat_1M.json"))
    args = ap.parse_args()

    import torch

    import bench
    from leann_amd import _lib
    from leann_amd.gpu_graph_build import _padded_table, build_graph_gpu
    from leann_amd.index import Mi355xIndex
    from leann_amd.pq import encode_pq_kernel, pq_scan_kernel, train_pq_kernel
    from leann_amd.recompute import RecomputeProvider
    from leann_amd.synth import CorpusSpec, SyntheticCorpus
    from leann_amd.token_store import TokenStore
    from leann_amd.index import allow_bitmap
    from oracle import oracle as orc

    def plan(ntotal, nq, m, L):
        """(queries per tile, slices, rows per slice): the slicing policy of include/leann_mi355x.h"""
        qt = min(8, (158 * 1024) // (1024 * m + 16 * L + 8 * 1280))
        nqt = max(1, -(-nq // qt))
        s0 = min(max(1, 512 // nqt), max(1, -(-ntotal // 2048)))
        rows = max(32, -(-(-(-ntotal // s0)) // 32) * 32)
        return qt, max(1, -(-ntotal // rows)), rows

    def scan_reference(cbh, ch, q, L):
        """inner product: orc_pq_lut, orc_pq_adc's order in fp32, keys (adc, id) ascending, distances negated"""
        labs, dists = [], []
        for qi in range(q.shape[0]):
            lut = orc.pq_lut_adc(cbh, ch, q[qi], 0, np.zeros(0, np.int64))[0]
            p = [np.zeros(ch.shape[0], np.float32) for _ in range(4)]
            for j in range(ch.shape[1]):
                p[j & 3] = p[j & 3] + lut[j][ch[:, j]]
            adc = (p[0] + p[1]) + (p[2] + p[3])
            adc = np.where(adc == 0, np.float32(0.0), adc).astype(np.float32)
            order = np.lexsort((np.arange(ch.shape[0]), adc))[:L]
            labs.append(order.astype(np.int64))
            dists.append(-adc[order])
        return np.stack(labs), np.stack(dists)

    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    t0 = time.time()
    corpus = SyntheticCorpus(CorpusSpec(n_chunks=args.chunks, seed=1234))
    enc = bench._load_encoder(args.model).to(dev, dtype=torch.float16).eval()
    tok, off = corpus.chunks()
    provider = RecomputeProvider(enc, TokenStore(tok, off, device=0), (enc.cfg.hidden + 63) // 64 * 64, dev)
    n = args.chunks
    X = torch.empty((n, enc.cfg.hidden), dtype=torch.float32, device=dev)
    for b0 in range(0, n, 32768):
        ids = torch.arange(b0, min(n, b0 + 32768), dtype=torch.int32, device=dev)
        X[b0 : b0 + ids.shape[0]] = provider.embed_ids(ids)
    qt, qo, _ = corpus.queries(64, seed=4321)
    Q = RecomputeProvider(enc, TokenStore(qt, qo, device=0), provider.dp, dev).embed_ids(torch.arange(64, dtype=torch.int32, device=dev)).contiguous()
    cb = train_pq_kernel(X, args.m, iters=8)
    codes = encode_pq_kernel(X, cb)
    torch.cuda.synchronize()
    print(f"[pq-flat-bench] {n} chunks embedded and quantised at m = {args.m} ({time.time() - t0:.1f}s)", flush=True)
    g = build_graph_gpu(X, "mips", M=32, ef_construction=200) if n >= 100_000 else build_graph_gpu(X, "mips", M=16, ef_construction=64)
    pruned = Mi355xIndex.from_csr(g, device=0)   # no table: codes + provider
    full = Mi355xIndex.from_csr(g, device=0)     # the table-carrying copy
    for idx in (pruned, full):
        idx.set_stream(torch.cuda.current_stream().cuda_stream)
        idx.attach_pq(cb.cpu().numpy(), codes.cpu().numpy())
    pruned.set_provider(provider)
    full.attach_table(_padded_table(X))
    print(f"[pq-flat-bench] graph built ({time.time() - t0:.1f}s)", flush=True)

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
    res = {"chunks": n, "d": int(X.shape[1]), "m": args.m, "k": k, "reps": args.reps, "warmup": args.warmup, "timing": "HIP events, median", "scan": {},
           "filtered": {}, "recall_at_k_vs_exact_filtered": {}}
    # correctness first: the first 20000 rows against the composed reference
    nc = min(n, 20000)
    dd, ll = pq_scan_kernel(codes[:nc], cb, Q[:2], args.L, "mips")
    assert nc >= args.L
    el, ed = scan_reference(cb.cpu().numpy(), codes[:nc].cpu().numpy(), np.ascontiguousarray(Q[:2].cpu().numpy()), args.L)
    assert np.array_equal(ll.cpu().numpy(), el) and np.array_equal(dd.cpu().numpy().view(np.uint32), ed.view(np.uint32)), "lm_pq_scan differs from the oracle's arithmetic"
    res["checked_against"] = f"oracle lookup table + ADC order on the first {nc} rows: labels and distance bits equal"
    code_bytes = codes.numel()
    for nq in (1, 8, 64):
        q = Q[:nq].contiguous()
        ms = timed(lambda: pq_scan_kernel(codes, cb, q, args.L, "mips"))
        res["scan"][str(nq)] = {"ms": ms, "code_bytes": code_bytes, "code_GBps": code_bytes / ms / 1e6, "plan_qt_S_rows": list(plan(n, nq, args.m, args.L))}
        print(f"[pq-flat-bench] scan nq={nq}: {json.dumps(res['scan'][str(nq)])}", flush=True)
    qraw = Q[: args.nq].contiguous()
    rng = np.random.default_rng(7)
    gprm = pruned.make_params(ef=args.ef, beam=1, recompute=True)
    for sel in (1.0, 0.1, 0.01, 0.001):
        mask = rng.random(n) < sel if sel < 1.0 else np.ones(n, bool)
        words = torch.from_numpy(allow_bitmap(mask, n).view(np.int32)).to(dev)
        fprm = pruned.make_pq_params(args.L, 1, use_deferred_fetch=True)
        xl = full.search_exact_device(qraw, k, allowed=words)[1].cpu().numpy()
        gl = pruned.search_device(qraw, k, gprm)[1].cpu().numpy()
        row = {"allowed_rows": int(mask.sum()),
               "pq_flat_ms": timed(lambda: pruned.pq_flat_search_device(qraw, k, fprm, allowed=words)),
               "graph_recompute_ef%d_ms" % args.ef: timed(lambda: pruned.search_device(qraw, k, gprm)),
               "graph_post_filter_mean_hits": float(np.mean([sum(1 for v in r if v >= 0 and mask[v]) for r in gl])),
               "exact_filtered_ms": timed(lambda: full.search_exact_device(qraw, k, allowed=words))}
        res["filtered"][str(sel)] = row
        rec = {}
        for L in (64, 256, 1024):
            fl = pruned.pq_flat_search_device(qraw, k, pruned.make_pq_params(L, 1, use_deferred_fetch=True), allowed=words)[0].cpu().numpy()
            rec[str(L)] = float(np.mean([len(set(a[a >= 0].tolist()) & set(b[b >= 0].tolist())) / max(1, int((b >= 0).sum())) for a, b in zip(fl, xl)]))
        res["recall_at_k_vs_exact_filtered"][str(sel)] = rec
        print(f"[pq-flat-bench] selectivity {sel}: {json.dumps(row)} recall {json.dumps(rec)}", flush=True)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
