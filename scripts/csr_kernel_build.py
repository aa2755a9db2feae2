#!/usr/bin/env python
"""Graph build and pruning time with the CSR assembled by numpy on the host (assembler="numpy": an export of every level, _assemble_csr;
in the pruning the dense level-0 array from the CSR and _with_level0) against the library's kernels (assembler="kernel":
lm_graph_levels_to_csr_count / _fill, lm_graph_csr_to_level), on the corpus bench.py builds its index over: the synthetic corpus
(seed 1234) embedded by the benchmark's encoder, M / ef_construction as bench.py passes them, selector, linker, inserter and pruner
"kernel" and search="view" throughout (DESIGN.md's view-search protocol).
One untimed warm-up build and pruning of 20 000 rows per assembler, then the assemblers alternating, --runs times each, every timed
region between device synchronisations: the whole build; inside it the final assembly alone (numpy: the level exports plus
_assemble_csr; kernel: assemble_csr_kernel, the host copy of the four arrays included); then the pruning call alone (m_low 8,
hub_fraction 0.02) on the graph just built.  Whether the built graphs, and the pruned ones, are byte-identical to the first is recorded.
"kernel" counts as faster only if its median lies outside the "numpy" runs' own min-max spread.  One JSON document.

    python scripts/csr_kernel_build.py --chunks 1000000 --out profiles/csr_kernel_build_1M.json
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
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--model", default="sentence-transformers/all-MiniLM-L6-v2")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()

    import torch

    import bench
    from leann_amd import _lib
    from leann_amd import gpu_graph_build as gb
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
    torch.cuda.synchronize()
    print(f"corpus embedded ({time.time() - t0:.1f} s)", flush=True)

    kw = dict(M=args.M, ef_construction=args.efc, selector="kernel", linker="kernel", search="view", inserter="kernel")
    modes = ("numpy", "kernel")
    log = []

    def timed(fn):
        def w(*a, **k):
            torch.cuda.synchronize()
            t = time.time()
            out = fn(*a, **k)
            torch.cuda.synchronize()
            log.append(time.time() - t)
            return out

        return w

    gb._LevelGraph.export = timed(gb._LevelGraph.export)
    gb._assemble_csr = timed(gb._assemble_csr)
    gb.assemble_csr_kernel = timed(gb.assemble_csr_kernel)

    def run(x, a):
        del log[:]
        torch.cuda.synchronize()
        t0 = time.time()
        g = gb.build_graph_gpu(x, "mips", assembler=a, **kw)
        torch.cuda.synchronize()
        t1 = time.time()
        asm = sum(log)
        p = gb.prune_preserving_hubs(g, x, args.M, args.m_low, 0.02, pruner="kernel", assembler=a)
        torch.cuda.synchronize()
        return g, p, round(t1 - t0, 3), round(asm, 3), round(time.time() - t1, 3)

    for a in modes:  # untimed warm-up: library load, allocator, kernel code upload
        run(X[:20000].contiguous(), a)

    def csr_bytes(g):
        return (g.ntotal, g.entry_point, g.max_level) + tuple(getattr(g, f).tobytes() for f in ("levels", "level_ptr", "node_offsets", "neighbors"))

    secs = {a: {"build_s": [], "assembly_s": [], "prune_s": []} for a in modes}
    first = None
    same_built = same_pruned = True
    links = {}
    for r in range(args.runs):
        for a in modes:  # alternating: drift of the machine hits both alike
            g, p, tb, ta, tp = run(X, a)
            for k, v in zip(("build_s", "assembly_s", "prune_s"), (tb, ta, tp)):
                secs[a][k].append(v)
            b = (csr_bytes(g), csr_bytes(p))
            first = first or b
            same_built, same_pruned = same_built and b[0] == first[0], same_pruned and b[1] == first[1]
            links = {"built": int(g.neighbors.shape[0]), "pruned": int(p.neighbors.shape[0]), "n_level_ptr": int(g.level_ptr.shape[0]), "max_level": int(g.max_level)}
            print(json.dumps({"run": r, "assembler": a, "build_s": tb, "assembly_s": ta, "prune_s": tp, "built_identical": b[0] == first[0], "pruned_identical": b[1] == first[1]}),
                  flush=True)
            del g, p, b

    def verdict(k):
        n, m = secs["numpy"][k], statistics.median(secs["kernel"][k])
        return "kernel faster (its median lies below every numpy run)" if m < min(n) else "kernel slower (its median lies above every numpy run)" if m > max(n) \
            else "no difference outside the numpy runs' own spread"

    summary = {a: {k: {"runs": v, "median": round(statistics.median(v), 3), "min": min(v), "max": max(v)} for k, v in secs[a].items()} for a in modes}
    doc = {"what": "build_graph_gpu + prune_preserving_hubs over the benchmark corpus, kernel selector / linker / inserter / pruner, view search: CSR assembly by numpy vs "
                   "lm_graph_levels_to_csr_count / _fill and lm_graph_csr_to_level",
           "chunks": args.chunks, "d": D, "M": args.M, "ef_construction": args.efc, "m_low": args.m_low, "hub_fraction": 0.02, "runs_per_assembler": args.runs,
           "device": torch.cuda.get_device_name(0), "built_graphs_byte_identical": bool(same_built), "pruned_graphs_byte_identical": bool(same_pruned), **links,
           "seconds": summary, "verdict": {k: verdict(k) for k in ("build_s", "assembly_s", "prune_s")},
           "not_measured": "the device-only time of _count + _fill (assembly_s includes the host copy of the four arrays), the 10M-chunk case"}
    print(json.dumps({"verdict": doc["verdict"], "built_identical": bool(same_built), "pruned_identical": bool(same_pruned)}), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
