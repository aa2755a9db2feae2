#!/usr/bin/env python
"""How many forwards should the library-side recompute provider keep in flight?  A forward is a chain of ~20 dependent launches, each of which
drains the chip before the next starts; with option "lanes" 2 or 3 (csrc/lm_recompute.hip) the provider runs a call's forwards side by
side on streams of its own, so one forward's last, partly filled round of workgroups runs beside a kernel of another.  This is the
product form of the `--streams` experiment of scripts/forward_size_ab.py (several Python providers on torch streams): ONE provider, ONE
call, the same list of chunks at every lane count, several seconds per setting, the settings interleaved, clocks and power sampled
alongside.  One JSON line per (round, setting); round 0 of a process carries its warm-up order effect and is not to be compared.

    python scripts/forward_lanes_ab.py [--chunks 400000] [--ids 350000] [--rounds 3] [--lanes 1,2,3] [--budget 1048512]
"""
import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch

import bench as B
from leann_amd.encoder import BertEncoder, config_for
from leann_amd.recompute import RecomputeProvider
from leann_amd.synth import CorpusSpec, SyntheticCorpus
from leann_amd.token_store import TokenStore

ap = argparse.ArgumentParser()
ap.add_argument("--chunks", type=int, default=400_000)
ap.add_argument("--ids", type=int, default=350_000)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--calls", type=int, default=2, help="calls per measurement (each embeds --ids chunks)")
ap.add_argument("--lanes", default="1,2,3")
ap.add_argument("--budget", type=int, default=1048512, help="tokens per forward (the product default: 5461 x 192)")
ap.add_argument("--split-ids", type=int, default=3000, help="also time calls of this many chunks (~540 k tokens: below the budget, so the call is SPLIT into parts -- "
                "the shape of a round of the 2048-query benchmark step); 0 = skip")
ap.add_argument("--model", default="sentence-transformers/all-MiniLM-L6-v2")
args = ap.parse_args()

dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
corpus = SyntheticCorpus(CorpusSpec(n_chunks=args.chunks, seed=1234))
tok, off = corpus.chunks()
tokens = TokenStore(tok, off, device=0)
cfg = config_for(args.model)
enc = BertEncoder.load(args.model, allow_random=True).to(dev, dtype=torch.float16).eval()
rng = np.random.default_rng(7)
ids_np = rng.permutation(args.chunks)[: args.ids].astype(np.int32)
ids = torch.from_numpy(ids_np).to(dev)
lanes = [int(x) for x in args.lanes.split(",")]
provider = RecomputeProvider(enc, tokens, (cfg.hidden + 63) // 64 * 64, dev, batch_size=args.budget // 192)
assert provider.native() is not None, "library-side provider expected"
shapes = [("budget", ids, args.calls)]
if args.split_ids:
    shapes.append(("split", ids[: args.split_ids].contiguous(), 40 * args.calls))

ref = {}
for ln in lanes:  # warm-up (allocations of every lane) + the outputs must not depend on the lane count
    provider.set_native_option("lanes", ln)
    for name, idl, _ in shapes:
        e = provider.embed_ids(idl)
        torch.cuda.synchronize()
        if name not in ref:
            ref[name] = e
        else:
            print(json.dumps({"shape": name, "lanes": ln, "max_abs_diff_to_first_setting": float((e - ref[name]).abs().max()), "bit_identical": bool(torch.equal(e, ref[name]))}), flush=True)
        del e
work = {}  # shape -> (tokens, algorithmic flops) of one call
for name, idl, _ in shapes:
    lens = (off[1:] - off[:-1])[idl.cpu().numpy()]
    work[name] = (int(lens.sum()), float(sum(cfg.flops_per_chunk(int(t)) for t in lens)))
for rnd in range(args.rounds):
    for name, idl, calls in shapes:
        n_tokens, flops = work[name]
        for ln in lanes:
            provider.set_native_option("lanes", ln)
            st0 = provider.native_stats()
            torch.cuda.synchronize()
            smp = B.BoxSampler(0, period_s=0.2).start()
            t0 = time.perf_counter()
            for _ in range(calls):
                provider.embed_ids(idl)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / calls
            box = smp.stop()
            st1 = provider.native_stats()
            print(json.dumps({"round": rnd, "shape": name, "lanes": ln, "forward_tokens_budget": args.budget, "forwards_per_call": (st1["forwards"] - st0["forwards"]) // calls,
                              "chunks": int(idl.shape[0]), "tokens": n_tokens, "ms_per_call": round(dt * 1e3, 2), "chunks_per_s": round(idl.shape[0] / dt),
                              "TFLOPs": round(flops / dt / 1e12, 1), "sclk_mhz": box.get("sclk_mhz"), "power_w": box.get("power_w")}), flush=True)
