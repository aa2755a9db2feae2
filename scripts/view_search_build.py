#!/usr/bin/env python
"""Graph build time with the per-batch CSR round trip (build_graph_gpu(search="csr"): host copy of every level's adjacency, numpy CSR
assembly, a fresh lm_index per insert batch) against the view index (search="view": lm_index_create_view, one handle per level that searches
the adjacencies where lm_graph_add_links keeps them), on the corpus bench.py builds its index over: the synthetic corpus (seed 1234)
embedded by the benchmark's encoder, M / ef_construction / seed as bench.py passes them, selector="kernel" and linker="kernel" throughout
(with them the two modes build the same graph).
One untimed warm-up build of 20 000 rows per mode, then the modes alternating, --runs builds each; per mode: build seconds of every run
(median, min, max), recall@10 at ef 64 of the stored-embedding search against the exact top 10 (bench.py's query seed), and whether every
graph's CSR arrays are byte-identical to the first.  Then ONE more "csr" build with a device synchronisation around the round trip's parts --
the adjacency exports, _assemble_csr, Mi355xIndex.from_csr, close -- which gives the seconds the view removes (that build's own build_s is
not an untimed figure and is reported apart).  "view" counts as faster only if its median lies outside the "csr" runs' own min-max spread.
One JSON document.

    python scripts/view_search_build.py --chunks 1000000 --out profiles/view_search_build_1M.json
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
    ap.add_argument("--queries", type=int, default=2048)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--model", default="sentence-transformers/all-MiniLM-L6-v2")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()

    import torch

    import bench
    from leann_amd import _lib
    from leann_amd import gpu_graph_build as gb
    from leann_amd.exact import exact_topk_ip
    from leann_amd.gpu_graph_build import build_graph_gpu
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

    kw = dict(M=args.M, ef_construction=args.efc, selector="kernel", linker="kernel")
    modes = ("csr", "view")
    for s in modes:  # untimed warm-up: library load, allocator, kernel code upload
        build_graph_gpu(X[:20000].contiguous(), "mips", search=s, **kw)
    torch.cuda.synchronize()

    def csr_bytes(g):
        return (g.ntotal, g.entry_point, g.max_level) + tuple(getattr(g, f).tobytes() for f in ("levels", "level_ptr", "node_offsets", "neighbors"))

    def recall(g):
        idx = Mi355xIndex.from_csr(g)
        tab = torch.zeros((args.chunks, idx.info.d_padded), dtype=torch.float32, device=dev)
        tab[:, :D] = X
        idx.attach_table(tab)
        _, lab = idx.search_device(Q, 10, idx.make_params(ef=64, recompute=False))
        torch.cuda.synchronize()
        lab = lab.cpu().numpy()
        idx.close()
        return float(sum(len(set(lab[i].tolist()) & set(gt[i].tolist())) for i in range(args.queries)) / (10 * args.queries))

    secs = {s: [] for s in modes}
    info = {}
    first = None
    same = True
    for r in range(args.runs):
        for s in modes:  # alternating: drift of the box hits both modes alike
            torch.cuda.synchronize()
            t0 = time.time()
            g = build_graph_gpu(X, "mips", search=s, **kw)
            torch.cuda.synchronize()
            secs[s].append(round(time.time() - t0, 2))
            b = csr_bytes(g)
            if first is None:
                first = b
            same = same and b == first
            if s not in info:
                info[s] = {"recall_at_10_ef64": round(recall(g), 4), "mean_degree0": round(float(g.level0_degrees().mean()), 2), "edges": int(g.neighbors.shape[0]),
                           "max_level": int(g.max_level)}
            print(json.dumps({"run": r, "search": s, "build_s": secs[s][-1], "identical_to_first": b == first}), flush=True)
            del g, b

    # the round trip's share: one more "csr" build, synchronised around each part
    log = []

    def timed(name, fn):
        def w(*a, **k):
            torch.cuda.synchronize()
            t = time.time()
            out = fn(*a, **k)
            torch.cuda.synchronize()
            log.append((name, time.time() - t))
            return out

        return w

    real = (gb._LevelGraph.export, gb._assemble_csr, Mi355xIndex.from_csr, Mi355xIndex.close)
    gb._LevelGraph.export = timed("export", real[0])
    gb._assemble_csr = timed("assemble", real[1])
    Mi355xIndex.from_csr = classmethod(timed("from_csr", real[2].__func__))
    Mi355xIndex.close = timed("close", real[3])
    try:
        torch.cuda.synchronize()
        t0 = time.time()
        build_graph_gpu(X, "mips", search="csr", **kw)
        torch.cuda.synchronize()
        timed_build_s = time.time() - t0
    finally:
        gb._LevelGraph.export, gb._assemble_csr, Mi355xIndex.from_csr, Mi355xIndex.close = real[0], real[1], real[2], real[3]
    last_close = max(i for i, (n, _) in enumerate(log) if n == "close")  # what follows is the final graph's assembly, which both modes do
    parts = {}
    for n, t in log[: last_close + 1]:
        parts[n] = parts.get(n, 0.0) + t
    round_trip = {"seconds": round(sum(parts.values()), 2), "parts_s": {n: round(t, 2) for n, t in parts.items()},
                  "searches": sum(1 for n, _ in log if n == "from_csr"), "final_assembly_s": round(sum(t for _, t in log[last_close + 1 :]), 2),
                  "build_s_of_this_synchronised_run": round(timed_build_s, 2)}
    print(json.dumps({"csr_round_trip": round_trip}), flush=True)

    summary = {s: {"build_s": secs[s], "median_s": round(statistics.median(secs[s]), 2), "min_s": min(secs[s]), "max_s": max(secs[s]), **info[s]} for s in modes}
    view_faster = summary["view"]["median_s"] < summary["csr"]["min_s"]
    view_slower = summary["view"]["median_s"] > summary["csr"]["max_s"]
    doc = {"what": "build_graph_gpu over the benchmark corpus, selector=kernel, linker=kernel: candidate search through a per-batch CSR index vs one view index per level",
           "chunks": args.chunks, "d": D, "M": args.M, "ef_construction": args.efc, "queries": args.queries, "runs_per_mode": args.runs,
           "device": torch.cuda.get_device_name(0), "csr_arrays_byte_identical": bool(same), "builds": summary,
           "verdict": "view faster (its median lies below every csr run)" if view_faster else "view slower (its median lies above every csr run)" if view_slower
           else "no difference outside the csr runs' own spread",
           "csr_round_trip": round_trip}
    print(json.dumps({"csr_arrays_byte_identical": bool(same), "verdict": doc["verdict"]}), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
