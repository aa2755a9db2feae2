#!/usr/bin/env python
"""Stored-embedding graph search at the wide padded widths (csrc/lm_wide_impl.h) on the MI355X: 1536 and 3072, fp16 and fp32 tables, with the
register-resident 1024-wide form on the same graph shape beside them.  Writes profiles/wide_table_search.json.

    python scripts/wide_table_bench.py [--rows 1000000] [--queries 8192 32768] [--calls 5] [--out profiles/wide_table_search.json]

The graph is synthetic and one level deep: a ring plus `--degree - 1` random links per node (the traversal's cost is row reads; what the rows
hold does not matter to it), rows and queries are unit-variance normal.  Rows: `--rows`, or the largest count whose table fits
`--table-gib`.  Per configuration: one warm-up call, then the median of `--calls` timed lm_index_search_device calls (host clock around a call
that ends in a stream synchronise), queries/s, and the ALGORITHMIC row bytes/s -- ndis x d_padded x element size over the call time -- as a
fraction of 8 TB/s.  That is a whole-call rate (graph gathers, visited bits, merges and launch included), not a kernel's share of peak.
The box: clocks and power sampled while the calls run, and a device copy rate, with bench.py's own probes."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
HBM_PEAK = 8.0e12


def ring_graph(n, degree, d, seed):
    from leann_amd.csr_format import HnswCsr

    rng = np.random.default_rng(seed)
    nb = rng.integers(0, n, (n, degree), dtype=np.int32)
    nb[:, 0] = (np.arange(n) + 1) % n
    level_ptr = np.zeros(2 * n, np.uint64)
    level_ptr[0::2] = np.arange(n, dtype=np.uint64) * degree
    level_ptr[1::2] = level_ptr[0::2] + degree
    return HnswCsr(d=d, ntotal=n, metric_type=0, levels=np.ones(n, np.int32), level_ptr=level_ptr, node_offsets=np.arange(n + 1, dtype=np.uint64) * 2,
                   neighbors=np.ascontiguousarray(nb.reshape(-1)), entry_point=0, max_level=0)


def main():
    import torch

    from bench import BoxSampler, _copy_rate
    from leann_amd import _lib
    from leann_amd.index import Mi355xIndex

    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--table-gib", type=float, default=48.0)
    ap.add_argument("--degree", type=int, default=16)
    ap.add_argument("--queries", type=int, nargs="+", default=[8192, 32768])
    ap.add_argument("--widths", type=int, nargs="+", default=[1024, 1536, 3072])
    ap.add_argument("--ef", type=int, default=64)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "wide_table_search.json"))
    args = ap.parse_args()
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    out = {"what": "lm_index_search_device, recompute = 0, persistent launch, beam 1, k 10", "efSearch": args.ef, "degree": args.degree, "hbm_peak_bytes_per_s": HBM_PEAK,
           "device": torch.cuda.get_device_name(0), "copy_rate_gb_per_s": round(_copy_rate(dev), 1), "runs": []}
    sampler = BoxSampler(0, period_s=0.25).start()
    for dp in args.widths:
        for f16 in (True, False):
            es = 2 if f16 else 4
            n = int(min(args.rows, args.table_gib * 2**30 // (dp * es)))
            idx = Mi355xIndex.from_csr(ring_graph(n, args.degree, dp, 5))
            idx.set_stream(torch.cuda.current_stream().cuda_stream)
            table = torch.empty((n, dp), dtype=torch.float16 if f16 else torch.float32, device=dev)
            gen = torch.Generator(device=dev).manual_seed(dp + es)
            for r0 in range(0, n, 1 << 16):  # in blocks: normal_ of a half tensor goes through an fp32 temporary
                table[r0 : r0 + (1 << 16)].normal_(generator=gen)
            idx.attach_table(table)
            prm = idx.make_params(ef=args.ef, beam=1, recompute=False, max_batch=max(args.queries))
            for nq in args.queries:
                q = torch.randn((nq, dp), device=dev, generator=gen)
                times = []
                for call in range(args.calls + 1):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    idx.search_device(q, 10, prm)
                    torch.cuda.synchronize()
                    if call:
                        times.append(time.perf_counter() - t0)
                st = idx.stats()
                med = float(np.median(times))
                row_bytes = int(st["ndis"]) * dp * es
                out["runs"].append({"d_padded": dp, "dtype": "f16" if f16 else "f32", "rows": n, "queries": nq, "calls_s": [round(t, 5) for t in times], "median_s": round(med, 5),
                                    "queries_per_s": round(nq / med, 1), "ndis": int(st["ndis"]), "nrounds": int(st["nrounds"]), "update_launches": int(st["update_launches"]),
                                    "row_bytes_per_s": round(row_bytes / med, 1), "fraction_of_hbm_peak": round(row_bytes / med / HBM_PEAK, 4)})
                print(json.dumps(out["runs"][-1]), flush=True)
            idx.close()
            del table
            torch.cuda.empty_cache()
    out["clocks_during_the_calls"] = sampler.stop()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print("wrote", args.out, flush=True)


if __name__ == "__main__":
    main()
