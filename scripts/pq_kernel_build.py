#!/usr/bin/env python
"""Times the product quantiser's two build steps in both forms on one MI355X: torch train_pq + encode_pq, then train_pq_kernel +
encode_pq_kernel (lm_pq_train / lm_pq_encode), train and encode separately, each after one warm-up, synchronised, as the median of 5.
Shapes: 1M x 384, m = 48 (the bench's quantiser) and 10M x 384, m = 96 (configuration C3; halved until the table and torch's
temporaries fit).  Reports per form the mean squared reconstruction error over the full set, for encode the achieved fp32 FMA rate as
a share of the vector fp32 peak, and the bytes read per vector.
    python scripts/pq_kernel_build.py [--out profiles/pq_kernel_build.json] [--shapes 1M,10M] [--forms torch,kernel] [--reps 5]
`--forms kernel --reps 1` is the run to put under `rocprofv3 --kernel-trace --stats` (tracing only)."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

# MI355X vector fp32 peak: 157.3 TFLOP/s (AMD Instinct MI355X data sheet, "peak single precision (FP32) vector") = 78.65e12 FMA/s
PEAK_FP32_FMA_PER_S = 157.3e12 / 2
SHAPES = {"1M": (1_000_000, 384, 48), "10M": (10_000_000, 384, 96)}


def make_data(torch, n, d, seed):
    """Clustered unit vectors generated on the device in blocks (2000 centres, sigma 0.35: tests/util.clustered's model)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    cent = torch.randn((2000, d), generator=g, device="cuda")
    x = torch.empty((n, d), device="cuda")
    for b0 in range(0, n, 1 << 20):
        b = min(1 << 20, n - b0)
        x[b0 : b0 + b] = cent[torch.randint(0, 2000, (b,), generator=g, device="cuda")] + 0.35 * torch.randn((b, d), generator=g, device="cuda")
        x[b0 : b0 + b] /= x[b0 : b0 + b].norm(dim=1, keepdim=True)
    return x


def timed(torch, fn, reps):
    out = fn()  # warm-up
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return out, statistics.median(ts), ts


def mse(torch, x, cb, codes):
    m, _, dsub = cb.shape
    tot = torch.zeros((), dtype=torch.float64, device=x.device)
    ar = torch.arange(m, device=x.device)[None, :]
    for b0 in range(0, x.shape[0], 1 << 18):
        rec = cb[ar, codes[b0 : b0 + (1 << 18)].long()].reshape(-1, m * dsub)
        tot += ((x[b0 : b0 + (1 << 18)] - rec) ** 2).sum(dtype=torch.float64)
    return float(tot / x.shape[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/pq_kernel_build.json")
    ap.add_argument("--shapes", default="1M,10M")
    ap.add_argument("--forms", default="torch,kernel")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=12)
    a = ap.parse_args()
    import torch

    from leann_amd import _lib
    from leann_amd.pq import encode_pq, encode_pq_kernel, train_pq, train_pq_kernel

    _lib.require_gpu()
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "train_iters": a.iters, "train_sample": 131072,
           "peak_fp32_fma_per_s": PEAK_FP32_FMA_PER_S, "peak_source": "MI355X data sheet: 157.3 TFLOP/s peak vector fp32 = 78.65e12 FMA/s", "shapes": []}
    forms = {"torch": (train_pq, encode_pq), "kernel": (train_pq_kernel, encode_pq_kernel)}
    for name in a.shapes.split(","):
        n, d, m = SHAPES[name]
        note = None
        while True:
            try:
                x = make_data(torch, n, d, 1)
                break
            except torch.cuda.OutOfMemoryError:
                note = f"{SHAPES[name][0]} rows did not fit; halved"
                n //= 2
        row = {"name": name, "n": n, "d": d, "m": m, "note": note, "forms": {}}
        for form in a.forms.split(","):
            tr, en = forms[form]
            cb, t_train, ts_train = timed(torch, lambda: tr(x, m, iters=a.iters, seed=0), a.reps)
            codes, t_enc, ts_enc = timed(torch, lambda: en(x, cb), a.reps)
            fma = n * d * 256
            read = d * 4 if form == "kernel" else d * 4 + 2 * m * 256 * 4  # torch: the row + its [m, 256] fp32 scores written and read back
            row["forms"][form] = {
                "train_s": t_train, "train_s_all": ts_train, "encode_s": t_enc, "encode_s_all": ts_enc, "mse": mse(torch, x, cb, codes),
                "encode_fma_per_s": fma / t_enc, "encode_share_of_fp32_vector_peak": fma / t_enc / PEAK_FP32_FMA_PER_S,
                "encode_bytes_moved_per_vector": read + m,
            }
            print(name, form, json.dumps(row["forms"][form]), flush=True)
            del cb, codes
        res["shapes"].append(row)
        del x
        torch.cuda.empty_cache()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
