#!/usr/bin/env python
"""Hub-preserving pruning (LEANN paper, Algorithm 3) on the host against the library call: prune_preserving_hubs(pruner="torch") -- numpy
in-degrees and hub choice, torch link weights, add_links in chunks -- and pruner="kernel" (lm_graph_prune_hubs, one call on the device),
on the corpus bench.py builds its index over: the synthetic corpus (seed 1234) embedded by the benchmark's encoder.  The graph is built
ONCE (M / ef_construction as bench.py passes them, selector="kernel", linker="kernel", search="view"); both pruners then run on it with
selector="kernel" and linker="kernel", alternating, --runs synchronised runs each, at --m-low and --hub-fraction, after one untimed run of
each on 20 000 rows.  Both forms include what they need around the device work: the dense level-0 array built from the CSR, its upload
(kernel form), the new CSR's assembly.  Per form: the seconds of every run (median, min, max), mean level-0 degree and recall@10 at ef 64
of the stored-embedding search against the exact top 10 (bench.py's query seed); whether the kernel form's results are byte-identical.
The kernel form counts as faster only if its median lies outside the torch form's own min-max spread.  One JSON document.

    python scripts/prune_kernel_bench.py --chunks 1000000 --out profiles/prune_kernel_1M.json
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=1_000_000)
    ap.add_argument("--M", type=int, default=32)
    ap.add_argument("--efc", type=int, default=200)
    ap.add_argument("--m-low", type=int, default=8)
    ap.add_argument("--hub-fraction", type=float, default=0.02)
    ap.add_argument("--queries", type=int, default=2048)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--model", default="sentence-transformers/all-MiniLM-L6-v2")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()

    import torch

    import bench
    from leann_amd import _lib
    from leann_amd.exact import exact_topk_ip
    from leann_amd.gpu_graph_build import build_graph_gpu, prune_preserving_hubs
    from leann_amd.index import Mi355xIndex
    from leann_amd.recompute import RecomputeProvider
    from leann_amd.synth import CorpusSpec, SyntheticCorpus
    from leann_amd.token_store import TokenStore

    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    t0 = time.time()
    corpus = SyntheticCorpus(CorpusSpec(n_chunks=args.chunks, seed=1234))
    tok, off = corpus.chunks()
    enc = bench._load_encoder(args.model).to(dev, dtype=torch.float16).eval()
    D = enc.cfg.hidden
    prov = RecomputeProvider(enc, TokenStore(tok, off, device=0), (D + 63) // 64 * 64, dev)
    X = torch.empty((args.chunks, D), dtype=torch.float32, device=dev)
    for b0 in range(0, args.chunks, 32768):
        ids = torch.arange(b0, min(args.chunks, b0 + 32768), dtype=torch.int32, device=dev)
        X[b0 : b0 + ids.shape[0]] = prov.embed_ids(ids)
    qt, qo, _ = corpus.queries(args.queries, seed=4321)
    Q = RecomputeProvider(enc, TokenStore(qt, qo, device=0), prov.dp, dev).embed_ids(torch.arange(args.queries, dtype=torch.int32, device=dev)).contiguous()
    _, gt = exact_topk_ip(Q, X, 10)
    gt = gt.cpu().numpy()
    torch.cuda.synchronize()
    print(f"corpus embedded, ground truth ready ({time.time() - t0:.1f} s)", flush=True)

    kw = dict(M=args.M, ef_construction=args.efc, selector="kernel", linker="kernel", search="view")
    pk = dict(M=args.M, m_low=args.m_low, hub_fraction=args.hub_fraction, selector="kernel", linker="kernel")
    forms = ("torch", "kernel")
    small = X[:20000].contiguous()
    gs = build_graph_gpu(small, "mips", **kw)
    for f in forms:  # untimed warm-up: library load, allocator, kernel code upload
        prune_preserving_hubs(gs, small, pruner=f, **pk)
    torch.cuda.synchronize()
    t0 = time.time()
    g = build_graph_gpu(X, "mips", **kw)
    torch.cuda.synchronize()
    build_s = round(time.time() - t0, 2)
    print(json.dumps({"build_s": build_s, "mean_degree0": round(float(g.level0_degrees().mean()), 2)}), flush=True)

    def csr_bytes(p):
        return (p.ntotal, p.entry_point, p.max_level) + tuple(getattr(p, f).tobytes() for f in ("levels", "level_ptr", "node_offsets", "neighbors"))

    def recall(p):
        idx = Mi355xIndex.from_csr(p)
        tab = torch.zeros((args.chunks, idx.info.d_padded), dtype=torch.float32, device=dev)
        tab[:, :D] = X
        idx.attach_table(tab)
        _, lab = idx.search_device(Q, 10, idx.make_params(ef=64, recompute=False))
        torch.cuda.synchronize()
        lab = lab.cpu().numpy()
        idx.close()
        return float(sum(len(set(lab[i].tolist()) & set(gt[i].tolist())) for i in range(args.queries)) / (10 * args.queries))

    secs = {f: [] for f in forms}
    info = {}
    first_kernel = None
    kernel_same = True
    for r in range(args.runs):
        for f in forms:  # alternating: drift of the box hits both forms alike
            torch.cuda.synchronize()
            t0 = time.time()
            p = prune_preserving_hubs(g, X, pruner=f, **pk)
            torch.cuda.synchronize()
            secs[f].append(round(time.time() - t0, 3))
            if f == "kernel":
                b = csr_bytes(p)
                if first_kernel is None:
                    first_kernel = b
                kernel_same = kernel_same and b == first_kernel
                del b
            if f not in info:
                info[f] = {"recall_at_10_ef64": round(recall(p), 4), "mean_degree0": round(float(p.level0_degrees().mean()), 2), "edges": int(p.neighbors.shape[0])}
            print(json.dumps({"run": r, "pruner": f, "prune_s": secs[f][-1]}), flush=True)
            del p

    summary = {f: {"prune_s": secs[f], "median_s": round(statistics.median(secs[f]), 3), "min_s": min(secs[f]), "max_s": max(secs[f]), **info[f]} for f in forms}
    faster = summary["kernel"]["median_s"] < summary["torch"]["min_s"]
    slower = summary["kernel"]["median_s"] > summary["torch"]["max_s"]
    doc = {"what": "prune_preserving_hubs on one graph of the benchmark corpus (selector=kernel, linker=kernel): the host form (pruner=torch) vs lm_graph_prune_hubs (pruner=kernel)",
           "chunks": args.chunks, "d": D, "M": args.M, "ef_construction": args.efc, "m_low": args.m_low, "hub_fraction": args.hub_fraction, "queries": args.queries,
           "runs_per_form": args.runs, "device": torch.cuda.get_device_name(0), "graph_build_s": build_s,
           "unpruned": {"recall_at_10_ef64": round(recall(g), 4), "mean_degree0": round(float(g.level0_degrees().mean()), 2), "edges": int(g.neighbors.shape[0])},
           "forms": summary, "torch_spread_s": round(summary["torch"]["max_s"] - summary["torch"]["min_s"], 3), "kernel_results_byte_identical": bool(kernel_same),
           "verdict": "kernel form faster (its median lies below every torch run)" if faster else "kernel form slower (its median lies above every torch run)" if slower
           else "no difference outside the torch runs' own spread"}
    print(json.dumps({"kernel_results_byte_identical": bool(kernel_same), "verdict": doc["verdict"], "forms": summary}), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
