#!/usr/bin/env python
"""The filtered graph search (lm_index_search_filtered) next to the unfiltered one (lm_index_search) on the benchmark's synthetic corpus (the
chunks, encoder, graph builder, queries and search parameters of bench.py at its defaults: 1M chunks, M = 32, efSearch 64, beam 1, k = 10,
batches of 2048 queries), recompute through the library-side provider -- the pruned-HNSW index that has neither a stored table nor PQ codes.
  queries/s   of lm_index_search_device and of lm_index_search_filtered_device at allow densities 1.0, 0.1 and 0.01 (--steps timed calls after
              --warmup, each on its own batch of queries; wall clock around a synchronised call, median);
  short       the fraction of queries that come back with fewer than k hits at each density, under filtering and under post-filtering (the
              unfiltered result with the disallowed labels dropped), and the mean number of hits of either.
No threshold: the yardstick is the unfiltered search in the same process.  Before anything is timed, density 1.0 must return lm_index_search's
labels and distance bits, and a filtered call must leave (ndis, nexpand, nrounds, nunique) as the unfiltered call leaves them.
    python scripts/filtered_search_bench.py [--chunks 1000000] [--out profiles/filtered_search_1M.json]"""
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
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--ef", type=int, default=64)
    ap.add_argument("--beam", type=int, default=1)
    ap.add_argument("--M", type=int, default=32)
    ap.add_argument("--efc", type=int, default=200)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "filtered_search_1M.json"))
    args = ap.parse_args()

    import torch

    import bench
    from leann_amd import _lib
    from leann_amd.gpu_graph_build import build_graph_gpu
    from leann_amd.index import Mi355xIndex, allow_bitmap
    from leann_amd.recompute import RecomputeProvider
    from leann_amd.synth import CorpusSpec, SyntheticCorpus
    from leann_amd.token_store import TokenStore

    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    t0 = time.time()
    n, B, k = args.chunks, args.batch, args.k
    corpus = SyntheticCorpus(CorpusSpec(n_chunks=n, seed=1234))
    enc = bench._load_encoder(args.model).to(dev, dtype=torch.float16).eval()
    tok, off = corpus.chunks()
    provider = RecomputeProvider(enc, TokenStore(tok, off, device=0), (enc.cfg.hidden + 63) // 64 * 64, dev)
    X = torch.empty((n, enc.cfg.hidden), dtype=torch.float32, device=dev)
    for b0 in range(0, n, 32768):
        ids = torch.arange(b0, min(n, b0 + 32768), dtype=torch.int32, device=dev)
        X[b0 : b0 + ids.shape[0]] = provider.embed_ids(ids)[:, : enc.cfg.hidden]
    nbatches = args.steps + args.warmup
    nq = B * nbatches
    qt, qo, _ = corpus.queries(nq, seed=4321)
    Q = RecomputeProvider(enc, TokenStore(qt, qo, device=0), provider.dp, dev).embed_ids(torch.arange(nq, dtype=torch.int32, device=dev))[:, : enc.cfg.hidden].contiguous()
    torch.cuda.synchronize()
    print(f"[filtered-bench] {n} chunks and {nq} queries embedded ({time.time() - t0:.1f}s)", flush=True)
    g = build_graph_gpu(X, "mips", M=args.M, ef_construction=args.efc) if n >= 100_000 else build_graph_gpu(X, "mips", M=16, ef_construction=64)
    del X
    idx = Mi355xIndex.from_csr(g, device=0)  # pruned: no table, no PQ codes
    idx.set_stream(torch.cuda.current_stream().cuda_stream)
    idx.set_provider(provider)
    assert idx.native_provider, "the library-side provider did not attach"
    print(f"[filtered-bench] graph built ({time.time() - t0:.1f}s)", flush=True)
    prm = idx.make_params(ef=args.ef, beam=args.beam, recompute=True, max_batch=B)

    def stats():
        st = idx.stats()
        return [int(st[f]) for f in ("ndis", "nexpand", "nrounds", "nunique")]

    def timed(fn):
        """median seconds per call over the timed batches, and every batch's labels"""
        secs, labels = [], []
        for b in range(nbatches):
            q = Q[b * B : (b + 1) * B].contiguous()
            torch.cuda.synchronize()
            t = time.perf_counter()
            _, lab = fn(q)
            torch.cuda.synchronize()
            if b >= args.warmup:
                secs.append(time.perf_counter() - t)
                labels.append(lab.cpu().numpy())
        return statistics.median(secs), np.concatenate(labels)

    # correctness first
    q0 = Q[:64].contiguous()
    du, lu = idx.search_device(q0, k, prm)
    su = stats()
    ones = torch.from_numpy(allow_bitmap(np.ones(n, bool), n).view(np.int32)).to(dev)
    df, lf = idx.search_filtered_device(q0, k, prm, allowed=ones)
    assert torch.equal(lu, lf) and torch.equal(du.view(torch.int32), df.view(torch.int32)), "an all-ones allow-list must give lm_index_search's bits"
    assert stats() == su, "a filtered call must leave the stats of the unfiltered one"
    res = {"chunks": n, "d": int(enc.cfg.hidden), "M": args.M, "ef_search": args.ef, "beam": args.beam, "k": k, "batch": B, "steps": args.steps,
           "warmup": args.warmup, "timing": "wall clock around a synchronised call, median over the timed batches",
           "checked": "all-ones allow-list: labels and distance bits of lm_index_search on 64 queries; stats equal", "density": {}}
    sec_u, lab_u = timed(lambda q: idx.search_device(q, k, prm))
    res["unfiltered_qps"] = B / sec_u
    print(f"[filtered-bench] lm_index_search: {B / sec_u:.1f} queries/s", flush=True)
    rng = np.random.default_rng(7)
    for dens in (1.0, 0.1, 0.01):
        mask = rng.random(n) < dens if dens < 1.0 else np.ones(n, bool)
        words = torch.from_numpy(allow_bitmap(mask, n).view(np.int32)).to(dev)
        sec_f, lab_f = timed(lambda q: idx.search_filtered_device(q, k, prm, allowed=words))
        evals = idx.get_option("filtered_allowed_evals")
        hits_f = (lab_f >= 0).sum(1)
        hits_p = np.array([sum(1 for v in r if v >= 0 and mask[v]) for r in lab_u])
        row = {"allowed_nodes": int(mask.sum()), "filtered_qps": B / sec_f, "filtered_over_unfiltered": sec_u / sec_f,
               "allowed_evals_per_query_last_batch": evals / B,
               "fewer_than_k_filtered": float((hits_f < k).mean()), "fewer_than_k_post_filtered": float((hits_p < k).mean()),
               "mean_hits_filtered": float(hits_f.mean()), "mean_hits_post_filtered": float(hits_p.mean())}
        res["density"][str(dens)] = row
        print(f"[filtered-bench] density {dens}: {json.dumps(row)}", flush=True)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
