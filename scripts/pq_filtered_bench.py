#!/usr/bin/env python
"""The filtered PQ traversal (lm_pq_batch_search_filtered) on the synthetic corpus and index of scripts/bench_c3.py at C3's shape (bge-small
stand-in encoder, mean pooling, flat graph of degree <= 64 built with M = 32 / ef_construction 200, m = 96 PQ bytes, W = 64, L = 256, k = 10,
1024 queries per call): HIP-event time per call, median of --reps after --warmup.  The exact rerank reads a stored fp32 table.
  routes      at 100 % / 50 % / 10 % / 1 % allowed: lm_pq_batch_search_filtered; lm_pq_batch_search followed by a post-filter of its k results;
              lm_pq_flat_search at 16 queries -- the time per query and the mean number of hits returned, each.
  unfiltered  lm_pq_batch_search (PQ order: the traversal, its stats and the finalize) with --parent-lib (the library built from the parent
              commit) and with this tree's library, one child process per build, the two alternating rep by rep inside this call; the margin is
              the parent build's own min-max spread.  Skipped without --parent-lib.
Before anything is timed the filtered call is compared on the first --check-queries queries with the reference composed from the oracle
(tests/pq_filtered_ref_util.py): labels, distance bits, counts and "filtered_allowed_evals", at 50 % and 1 % allowed, PQ order and table rerank.
    python scripts/pq_filtered_bench.py [--chunks 1000000] [--parent-lib path/to/parent/libleann_mi355x.so] [--out profiles/pq_filtered_1M.json]"""
import argparse
import ctypes as C
import json
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def child(lib_path: str, data: str, L: int, W: int, k: int, threads: int):
    """One build of the library on the saved index: answers every line "go" on stdin with one timed lm_pq_batch_search_device call (ms)."""
    import torch

    from leann_amd._lib import PqSearchParams

    lib = C.CDLL(lib_path)
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    lib.lm_last_error.restype = C.c_char_p
    lib.lm_index_create_from_csr.argtypes = [i64, i32, i32, vp, vp, i64, vp, i64, vp, i32, i32, C.c_int, C.POINTER(vp)]
    lib.lm_index_free.argtypes = [vp]
    lib.lm_index_set_stream.argtypes = [vp, vp]
    lib.lm_index_set_option.argtypes = [vp, C.c_char_p, i64]
    lib.lm_pq_attach.argtypes = [vp, i32, vp, vp, i64]
    lib.lm_pq_search_params_default.argtypes = [C.POINTER(PqSearchParams)]
    lib.lm_pq_search_params_default.restype = None
    lib.lm_pq_batch_search_device.argtypes = [vp, i64, vp, i32, C.POINTER(PqSearchParams), vp, vp]
    z = {f.stem: np.load(f) for f in Path(data).glob("*.npy")}
    meta = json.loads((Path(data) / "meta.json").read_text())
    h = vp()

    def ok(rc, what):
        if rc != 0:
            raise RuntimeError(f"{what}: {lib.lm_last_error().decode()}")

    p = lambda a: a.ctypes.data_as(vp)  # noqa: E731
    ok(lib.lm_index_create_from_csr(meta["n"], meta["d"], meta["metric"], p(z["node_offsets"]), p(z["level_ptr"]), z["level_ptr"].size, p(z["neighbors"]),
                                    z["neighbors"].size, p(z["levels"]), meta["entry_point"], meta["max_level"], 0, C.byref(h)), "create")
    ok(lib.lm_index_set_stream(h, torch.cuda.current_stream().cuda_stream), "stream")
    ok(lib.lm_pq_attach(h, z["codebooks"].shape[0], p(z["codebooks"]), p(z["codes"]), z["codes"].shape[0]), "pq_attach")
    ok(lib.lm_index_set_option(h, b"pq_threads", threads), "pq_threads")
    prm = PqSearchParams()
    lib.lm_pq_search_params_default(C.byref(prm))
    prm.complexity, prm.beam_width, prm.skip_search_reorder = L, W, 1
    Q = torch.from_numpy(z["queries"]).cuda().contiguous()
    lab = torch.empty((Q.shape[0], k), dtype=torch.int64, device="cuda")
    dist = torch.empty((Q.shape[0], k), dtype=torch.float32, device="cuda")
    print("ready", flush=True)
    for line in sys.stdin:
        if line.strip() != "go":
            break
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ok(lib.lm_pq_batch_search_device(h, Q.shape[0], vp(Q.data_ptr()), k, C.byref(prm), vp(lab.data_ptr()), vp(dist.data_ptr())), "search")
        b.record()
        b.synchronize()
        print(json.dumps({"ms": a.elapsed_time(b), "label_sum": int(lab.sum().item())}), flush=True)
    lib.lm_index_free(h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=1_000_000)
    ap.add_argument("--model", default="BAAI/bge-small-en-v1.5")
    ap.add_argument("--m", type=int, default=96)
    ap.add_argument("--M", type=int, default=32, help="graph degree / 2 of the flat graph (degree <= 64, as C3 is measured)")
    ap.add_argument("--efc", type=int, default=200)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--L", type=int, default=256)
    ap.add_argument("--W", type=int, default=64)
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--flat-nq", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--check-queries", type=int, default=2)
    ap.add_argument("--pq-threads", type=int, default=1024, choices=[256, 512, 1024])
    ap.add_argument("--parent-lib", default="", help="libleann_mi355x.so built from the parent commit: times the unfiltered path with both builds")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "pq_filtered_1M.json"))
    ap.add_argument("--child", nargs=2, metavar=("LIB", "DATA"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], args.child[1], args.L, args.W, args.k, args.pq_threads)

    from dataclasses import replace

    import torch

    from leann_amd import _lib
    from leann_amd.encoder import BertEncoder, config_for
    from leann_amd.gpu_graph_build import _padded_table, build_graph_gpu
    from leann_amd.index import Mi355xIndex, allow_bitmap
    from leann_amd.pq import encode_pq, flat_graph, train_pq
    from leann_amd.recompute import RecomputeProvider
    from leann_amd.synth import CorpusSpec, SyntheticCorpus
    from leann_amd.token_store import TokenStore
    from tests import pq_filtered_ref_util as pr

    def log(*a):
        print("[pq-filtered-bench]", *a, flush=True)

    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    n, k, L, W = args.chunks, args.k, args.L, args.W
    t0 = time.time()
    corpus = SyntheticCorpus(CorpusSpec(n_chunks=n, seed=1234, n_topics=max(1000, n // 1000)))
    tok, off = corpus.chunks_torch(dev)
    enc = BertEncoder.load(args.model, allow_random=True).to(dev, dtype=torch.float16).eval()
    if enc.weights_source == "random":
        enc.cfg = replace(enc.cfg, pooling="mean")  # as scripts/bench_c3.py: the stand-in encoder's [CLS] rows carry no topic signal
    D = config_for(args.model).hidden
    provider = RecomputeProvider(enc, TokenStore(tok, off), (D + 63) // 64 * 64, dev)
    X = torch.empty((n, D), dtype=torch.float32, device=dev)
    for b0 in range(0, n, 32768):
        ids = torch.arange(b0, min(n, b0 + 32768), dtype=torch.int32, device=dev)
        X[b0 : b0 + ids.shape[0]] = provider.embed_ids(ids)
    qt, qo, _ = corpus.queries(args.nq, seed=4321)
    Q = RecomputeProvider(enc, TokenStore(qt, qo), provider.dp, dev).embed_ids(torch.arange(args.nq, dtype=torch.int32, device=dev)).contiguous()
    log(f"{n} chunks embedded ({time.time() - t0:.0f}s)")
    fg = flat_graph(build_graph_gpu(X, "mips", M=args.M, ef_construction=args.efc), X)
    cb = train_pq(X, args.m, iters=10)
    codes = encode_pq(X, cb)
    cbh, ch = cb.cpu().numpy(), codes.cpu().numpy()
    idx = Mi355xIndex.from_csr(fg)
    idx.set_stream(torch.cuda.current_stream().cuda_stream)
    idx.attach_pq(cbh, ch)
    idx.attach_table(_padded_table(X))
    idx.set_option("pq_threads", args.pq_threads)
    deg0 = int(idx.info.max_degree0)
    log(f"flat graph (max level-0 degree {deg0}, mean {fg.level0_degrees().mean():.1f}) and PQ m = {args.m} ready ({time.time() - t0:.0f}s)")

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return statistics.median(ms)

    res = {"chunks": n, "d": D, "m": args.m, "max_degree0": deg0, "k": k, "L": L, "W": W, "queries_per_call": args.nq, "flat_queries_per_call": args.flat_nq,
           "pq_threads": args.pq_threads, "reps": args.reps, "warmup": args.warmup, "timing": "HIP events, median", "rerank": "stored fp32 table",
           "lds_bytes_filtered": pr.lds_bytes_filtered(deg0, args.m, L, W), "routes": {}}
    rng = np.random.default_rng(7)
    masks = {sel: (rng.random(n) < sel if sel < 1.0 else np.ones(n, bool)) for sel in (1.0, 0.5, 0.1, 0.01)}
    # correctness first: the first queries against the reference composed from the oracle
    if args.check_queries > 0:
        R = pr.Reference(fg, cbh, ch)
        qh = np.ascontiguousarray(Q[: args.check_queries].cpu().numpy()[:, :D])
        xh = X.cpu().numpy()
        for sel in (0.5, 0.01):
            for skip in (True, False):
                el, ed, eev, _, _, est = R.expected(qh, k, L, W, masks[sel], None if skip else xh)
                gl, gd = idx.pq_search_filtered(qh, k, idx.make_pq_params(L, W, skip_search_reorder=skip), allowed=masks[sel])
                st = idx.stats()
                assert pr.same(gl, gd, el, ed), f"filtered search differs from the reference at {sel} allowed, skip_search_reorder={skip}"
                assert (int(st["ndis"]), int(st["nexpand"]), int(st["nrounds"])) == est and idx.get_option("filtered_allowed_evals") == eev, (st, est, eev)
        del xh
        res["checked_against"] = (f"reference composed from the oracle on the first {args.check_queries} queries at 50 % and 1 % allowed, PQ order and table "
                                  "rerank: labels, distance bits, ndis / nexpand / nrounds and filtered_allowed_evals equal")
        log(res["checked_against"])
    Qd = Q[:, :D].contiguous()
    qflat = Qd[: args.flat_nq].contiguous()
    prm = idx.make_pq_params(L, W)
    plain_l = idx.pq_search_device(Qd, k, prm)[0].cpu().numpy()
    st = idx.stats()
    res["unfiltered_ndis_per_query"] = int(st["ndis"]) / args.nq
    for sel, mask in masks.items():
        words = torch.from_numpy(allow_bitmap(mask, n).view(np.int32)).to(dev)
        fl = idx.pq_search_filtered_device(Qd, k, prm, allowed=words)[0].cpu().numpy()
        evals = idx.get_option("filtered_allowed_evals")
        sl = idx.pq_flat_search_device(qflat, k, prm, allowed=words)[0].cpu().numpy()
        ms_f = timed(lambda: idx.pq_search_filtered_device(Qd, k, prm, allowed=words))
        ms_p = timed(lambda: idx.pq_search_device(Qd, k, prm))
        ms_s = timed(lambda: idx.pq_flat_search_device(qflat, k, prm, allowed=words))
        row = {"allowed_rows": int(mask.sum()), "allowed_evals_per_query": evals / args.nq,
               "traversal_filtered": {"ms_per_call": ms_f, "us_per_query": 1e3 * ms_f / args.nq, "mean_hits": float((fl >= 0).sum(1).mean())},
               "traversal_then_post_filter": {"ms_per_call": ms_p, "us_per_query": 1e3 * ms_p / args.nq,
                                              "mean_hits": float(np.mean([sum(1 for v in r if v >= 0 and mask[v]) for r in plain_l]))},
               "flat_scan": {"ms_per_call": ms_s, "us_per_query": 1e3 * ms_s / args.flat_nq, "mean_hits": float((sl >= 0).sum(1).mean())}}
        res["routes"][str(sel)] = row
        log(f"allowed {sel}: {json.dumps(row)}")
    if args.parent_lib:
        with tempfile.TemporaryDirectory() as td:
            for name, arr in (("node_offsets", fg.node_offsets), ("level_ptr", fg.level_ptr), ("neighbors", fg.neighbors), ("levels", fg.levels),
                              ("codebooks", cbh), ("codes", ch), ("queries", Qd.cpu().numpy())):
                np.save(Path(td) / f"{name}.npy", np.ascontiguousarray(arr))
            (Path(td) / "meta.json").write_text(json.dumps(dict(n=n, d=D, metric=int(fg.metric_type), entry_point=int(fg.entry_point), max_level=int(fg.max_level))))
            idx.close()
            del X, codes
            torch.cuda.empty_cache()
            builds = {"parent": args.parent_lib, "this": str(_lib.LIB_PATH)}
            procs = {}
            for name, lib in builds.items():
                cmd = [sys.executable, str(Path(__file__).resolve()), "--child", lib, td, "--L", str(L), "--W", str(W), "--k", str(k), "--pq-threads", str(args.pq_threads)]
                procs[name] = subprocess.Popen(cmd, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
            series = {name: [] for name in builds}
            sums = {name: set() for name in builds}
            try:
                for name, pr_ in procs.items():
                    assert pr_.stdout.readline().strip() == "ready", f"{name} build did not start"
                for rep in range(args.warmup + args.reps):
                    for name, pr_ in procs.items():  # alternating: parent, this, parent, this ...
                        pr_.stdin.write("go\n")
                        pr_.stdin.flush()
                        got = json.loads(pr_.stdout.readline())
                        sums[name].add(got["label_sum"])
                        if rep >= args.warmup:
                            series[name].append(got["ms"])
            finally:
                for pr_ in procs.values():
                    pr_.stdin.close()
                    pr_.wait(timeout=120)
        assert sums["parent"] == sums["this"] and len(sums["this"]) == 1, "the two builds return different labels"
        pm, tm = statistics.median(series["parent"]), statistics.median(series["this"])
        lo, hi = min(series["parent"]), max(series["parent"])
        res["unfiltered_vs_parent"] = {"call": "lm_pq_batch_search_device, skip_search_reorder (traversal + stats + finalize)", "parent_ms": series["parent"],
                                       "this_ms": series["this"], "parent_median_ms": pm, "this_median_ms": tm, "parent_min_ms": lo, "parent_max_ms": hi,
                                       "this_median_inside_parent_spread": bool(lo <= tm <= hi), "same_labels": True}
        log(f"unfiltered: parent median {pm:.3f} ms (min {lo:.3f}, max {hi:.3f}), this build median {tm:.3f} ms")
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps({k2: v for k2, v in res.items() if k2 != "unfiltered_vs_parent"}))


if __name__ == "__main__":
    main()
