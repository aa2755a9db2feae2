#!/usr/bin/env python
"""Attention alone at head_dim 32, 12 heads, ~262 k tokens of sequences of 257..512 tokens: lm_attn_varlen_hd32_f16 (generation 3 + its long
form in one launch) against torch's varlen attention -- what the per-kernel forward fell back to for these lengths before the long form --
alternating in one process; for scale, generation 3 alone at uniform 256.  HIP events around `--iters` launches, `--runs` runs each, medians
and min-max.  Writes one JSON object (default profiles/attention_long_262k.json).
    python scripts/attention_long_bench.py"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=262144)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "attention_long_262k.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from torch.nn.attention.varlen import varlen_attn

    from leann_amd import _lib
    from leann_amd.encoder import fused_attention_hd32

    _lib.require_gpu()
    heads, rng = 12, np.random.default_rng(0)
    mixes = {"uniform 512": np.full(a.tokens // 512, 512), "N(380, 80) clipped to 257..512": np.clip(rng.normal(380, 80, a.tokens // 380).round(), 257, 512),
             "uniform 256 (generation 3 alone)": np.full(a.tokens // 256, 256)}

    def timed(fn):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(a.iters):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) * 1000.0 / a.iters

    res = {"command": " ".join(sys.argv), "device": torch.cuda.get_device_name(0), "heads": heads, "iters_per_run": a.iters, "mixes": {}}
    for name, lens in mixes.items():
        lens = lens.astype(np.int64)
        cu = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)).cuda()
        tot, mx = int(lens.sum()), int(lens.max())
        qkv = (torch.randn((tot, 3 * 32 * heads), device="cuda") * 1.5).half()
        q4 = qkv.view(tot, 3, heads, 32)
        forms = {"lm_attn_varlen_hd32_f16": lambda: fused_attention_hd32(qkv, cu, heads, mx),
                 "torch varlen_attn": lambda: varlen_attn(q4[:, 0], q4[:, 1], q4[:, 2], cu, cu, mx, mx)}
        diff = (forms["lm_attn_varlen_hd32_f16"]().float() - forms["torch varlen_attn"]().reshape(tot, -1).float()).abs().max().item()
        us = {k: [] for k in forms}
        for r in range(a.runs + 1):  # run 0 = warm-up
            for k, fn in forms.items():
                t = timed(fn)
                if r:
                    us[k].append(round(t, 1))
        row = {"sequences": len(lens), "tokens": tot, "max_abs_diff_between_the_two": diff}
        for k, v in us.items():
            row[k] = {"us_runs": v, "us_median": statistics.median(v), "us_min": min(v), "us_max": max(v), "ns_per_token": round(statistics.median(v) * 1000.0 / tot, 3)}
        res["mixes"][name] = row
        print(name, json.dumps(row), flush=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
