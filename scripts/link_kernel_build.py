#!/usr/bin/env python
"""Graph build time with the torch link insertion (_LevelGraph.add_links' torch-op composition) against the HIP kernels
(lm_graph_add_links), on the corpus bench.py builds its index over: the synthetic corpus (seed 1234) embedded by the benchmark's encoder,
M / ef_construction / seed as bench.py passes them, selector="kernel" throughout (with it the two linkers build the same graph).
One untimed warm-up build of 20 000 rows per linker, then each linker once at full size; per graph: build seconds, mean level-0 degree,
recall@10 at ef 64 of the stored-embedding search against the exact top 10 (bench.py's query seed); and whether the two graphs' CSR arrays
are byte-identical.  One JSON document.  The figure to beat is the torch linker's of the same run.

    python scripts/link_kernel_build.py --chunks 1000000 --out profiles/link_kernel_build_1M.json
    python scripts/link_kernel_build.py --chunks 1000000 --time-links --out <file>     # add_links' share: a device synchronisation around
                                                                                        # every call, so build_s is not the untimed figure
"""
import argparse
import json
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
    ap.add_argument("--model", default="sentence-transformers/all-MiniLM-L6-v2")
    ap.add_argument("--only", choices=("torch", "kernel"), default=None)
    ap.add_argument("--time-links", action="store_true", help="synchronise around every add_links call and record the seconds spent in it")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()

    import torch

    import bench
    from leann_amd import _lib
    from leann_amd.exact import exact_topk_ip
    from leann_amd import gpu_graph_build as gb
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

    linkers = [args.only] if args.only else ["kernel", "torch"]
    for s in linkers:  # untimed warm-up: library load, allocator, kernel code upload
        build_graph_gpu(X[:20000].contiguous(), "mips", M=args.M, ef_construction=args.efc, selector="kernel", linker=s)
    torch.cuda.synchronize()
    spent = {"s": 0.0, "calls": 0}
    if args.time_links:
        real = gb._LevelGraph.add_links

        def timed(self, *a, **k):
            torch.cuda.synchronize()
            t = time.time()
            r = real(self, *a, **k)
            torch.cuda.synchronize()
            spent["s"] += time.time() - t
            spent["calls"] += 1
            return r

        gb._LevelGraph.add_links = timed
    rows = []
    graphs = {}
    for s in linkers:
        spent.update(s=0.0, calls=0)
        t0 = time.time()
        g = build_graph_gpu(X, "mips", M=args.M, ef_construction=args.efc, selector="kernel", linker=s)
        torch.cuda.synchronize()
        sec = time.time() - t0
        graphs[s] = g
        idx = Mi355xIndex.from_csr(g)
        tab = torch.zeros((args.chunks, idx.info.d_padded), dtype=torch.float32, device=dev)
        tab[:, :D] = X
        idx.attach_table(tab)
        _, lab = idx.search_device(Q, 10, idx.make_params(ef=64, recompute=False))
        torch.cuda.synchronize()
        lab = lab.cpu().numpy()
        idx.close()
        del tab
        rec = float(sum(len(set(lab[i].tolist()) & set(gt[i].tolist())) for i in range(args.queries)) / (10 * args.queries))
        deg = g.level0_degrees()
        rows.append({"linker": s, "build_s": round(sec, 2), "recall_at_10_ef64": round(rec, 4), "mean_degree0": round(float(deg.mean()), 2),
                     "edges": int(g.neighbors.shape[0]), "max_level": int(g.max_level)})
        if args.time_links:
            rows[-1].update(add_links_s=round(spent["s"], 2), add_links_calls=spent["calls"])
        print(json.dumps(rows[-1]), flush=True)
    same = None
    if len(graphs) == 2:
        a, b = graphs["kernel"], graphs["torch"]
        same = bool(a.ntotal == b.ntotal and a.entry_point == b.entry_point and a.max_level == b.max_level
                    and all(getattr(a, f).tobytes() == getattr(b, f).tobytes() for f in ("levels", "level_ptr", "node_offsets", "neighbors")))
    doc = {"what": "build_graph_gpu over the benchmark corpus, selector=kernel: link insertion by torch ops vs lm_graph_add_links", "chunks": args.chunks, "d": D,
           "M": args.M, "ef_construction": args.efc, "queries": args.queries, "device": torch.cuda.get_device_name(0),
           "synchronised_around_add_links": bool(args.time_links), "csr_arrays_byte_identical": same, "builds": rows}
    print(json.dumps({"csr_arrays_byte_identical": same}), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
