#!/usr/bin/env python
"""The batched HNSW builder's insert step as torch ops between the kernels against one library call: build_graph_gpu(inserter="torch") and
inserter="kernel" (lm_graph_insert_batch), both with selector="kernel", linker="kernel", search="view", on the corpus bench.py builds its
index over: the synthetic corpus (seed 1234) embedded by the benchmark's encoder.  After one untimed 20 000-row build per form, the forms
alternate, --runs synchronised builds each.  Per form: the seconds of every build (median, min, max), recall@10 at ef 64 of the
stored-embedding search against the exact top 10 (bench.py's query seed) and the mean level-0 degree; whether all graphs are
byte-identical.  Then one more build per form under torch's synchronisation debug mode, which reports every torch op that makes the host
wait for the device: their number per insert call (the library's own waits -- the view search's counter read per pass and its closing
stream synchronisation -- are the same on both paths and are not torch ops).  The kernel form counts as faster only if its median lies
outside the torch form's own min-max spread.  One JSON document.

    python scripts/insert_kernel_bench.py --chunks 1000000 --out profiles/insert_kernel_1M.json

--only kernel --runs 1 --no-sync-count builds one form only (what a rocprofv3 --kernel-trace --stats run wraps, in a run of its own).
"""
import argparse
import json
import statistics
import sys
import time
import warnings
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=1_000_000)
    ap.add_argument("--M", type=int, default=32)
    ap.add_argument("--efc", type=int, default=200)
    ap.add_argument("--queries", type=int, default=2048)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--only", choices=("torch", "kernel"), default=None)
    ap.add_argument("--no-sync-count", action="store_true")
    ap.add_argument("--model", default="sentence-transformers/all-MiniLM-L6-v2")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()

    import torch

    import bench
    from leann_amd import _lib
    from leann_amd import gpu_graph_build as gb
    from leann_amd.exact import exact_topk_ip
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
    forms = (args.only,) if args.only else ("torch", "kernel")
    small = X[:20000].contiguous()
    for f in forms:  # untimed warm-up: library load, allocator, kernel code upload
        gb.build_graph_gpu(small, "mips", inserter=f, **kw)
    torch.cuda.synchronize()

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
    first = None
    same = True
    for r in range(args.runs):
        for f in forms:  # alternating: drift of the box hits both forms alike
            torch.cuda.synchronize()
            t0 = time.time()
            g = gb.build_graph_gpu(X, "mips", inserter=f, **kw)
            torch.cuda.synchronize()
            secs[f].append(round(time.time() - t0, 3))
            b = csr_bytes(g)
            if first is None:
                first = b
            same = same and b == first
            del b
            if f not in info:
                info[f] = {"recall_at_10_ef64": round(recall(g), 4), "mean_degree0": round(float(g.level0_degrees().mean()), 2), "edges": int(g.neighbors.shape[0])}
            print(json.dumps({"run": r, "inserter": f, "build_s": secs[f][-1]}), flush=True)
            del g

    syncs = {}
    if not args.no_sync_count:
        real_search, real_insert = gb._LevelView.search, gb._LevelView.insert
        for f in forms:  # untimed: every torch op that waits for the device warns once
            calls = [0]

            def search(self, *a, **k):
                calls[0] += 1
                return real_search(self, *a, **k)

            def insert(self, *a, **k):
                calls[0] += 1
                return real_insert(self, *a, **k)

            gb._LevelView.search, gb._LevelView.insert = search, insert
            torch.cuda.set_sync_debug_mode("warn")
            try:
                with warnings.catch_warnings(record=True) as w:
                    warnings.simplefilter("always")
                    gb.build_graph_gpu(X, "mips", inserter=f, **kw)
            finally:
                torch.cuda.set_sync_debug_mode("default")
                gb._LevelView.search, gb._LevelView.insert = real_search, real_insert
            n = sum(1 for x in w if "synchroniz" in str(x.message).lower())
            syncs[f] = {"insert_calls": calls[0], "torch_synchronising_ops_per_build": n, "per_insert_call": round(n / max(calls[0], 1), 2)}
            print(json.dumps({"inserter": f, **syncs[f]}), flush=True)

    summary = {f: {"build_s": secs[f], "median_s": round(statistics.median(secs[f]), 3), "min_s": min(secs[f]), "max_s": max(secs[f]), **info[f], **syncs.get(f, {})}
               for f in forms}
    verdict = None
    if len(forms) == 2:
        faster = summary["kernel"]["median_s"] < summary["torch"]["min_s"]
        slower = summary["kernel"]["median_s"] > summary["torch"]["max_s"]
        verdict = ("kernel form faster (its median lies below every torch run)" if faster else "kernel form slower (its median lies above every torch run)" if slower
                   else "no difference outside the torch runs' own spread")
    doc = {"what": "build_graph_gpu on the benchmark corpus (selector=kernel, linker=kernel, search=view): the insert step as torch ops (inserter=torch) vs "
                   "lm_graph_insert_batch (inserter=kernel)",
           "chunks": args.chunks, "d": D, "M": args.M, "ef_construction": args.efc, "queries": args.queries, "runs_per_form": args.runs,
           "device": torch.cuda.get_device_name(0), "forms": summary, "all_graphs_byte_identical": bool(same), "verdict": verdict,
           "host_synchronisations": "torch ops that make the host wait (torch.cuda.set_sync_debug_mode), one untimed build per form; the view search's own waits "
                                    "(one counter read per pass, one stream synchronisation per call) are the same on both paths and not counted"}
    print(json.dumps({"all_graphs_byte_identical": bool(same), "verdict": verdict, "forms": summary}), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
