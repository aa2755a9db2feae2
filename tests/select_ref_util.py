"""Helpers shared by the neighbour-selection tests (tests/test_select_neighbors.py on the CPU, tests/test_gpu_select_neighbors.py on the
MI355X): compile tests/select_ref/lm_select_ref.c -- the CPU restatement of lm_select_neighbors -- against the oracle library, call it on
numpy arrays, and generate candidate rows with every awkward feature the contract names."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
ORACLE_LIB = ROOT / "oracle" / "_build" / "liblm_oracle.so"


def compile_ref(out_dir: Path) -> Path:
    """gcc -O2 -ffp-contract=off, linked against the already built oracle (its orc_dist is the distance function)."""
    out = Path(out_dir) / "liblm_select_ref.so"
    subprocess.run(["gcc", "-std=c11", "-O2", "-ffp-contract=off", "-fopenmp", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror", "-o", str(out),
                    str(ROOT / "tests" / "select_ref" / "lm_select_ref.c"), f"-L{ORACLE_LIB.parent}", "-llm_oracle", "-lm",
                    f"-Wl,-rpath,{ORACLE_LIB.parent}"], check=True, capture_output=True)
    return out


def load_ref(path):
    lib = C.CDLL(str(path))
    lib.lm_select_ref.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_float, C.c_void_p]
    lib.lm_select_ref.restype = C.c_int
    return lib


def pad64(x: np.ndarray) -> np.ndarray:
    """[N, d] -> [N, d rounded up to a multiple of 64], zero padded, same dtype."""
    dp = (x.shape[1] + 63) // 64 * 64
    t = np.zeros((x.shape[0], dp), x.dtype)
    t[:, : x.shape[1]] = x
    return t


def ref_select(ref, table: np.ndarray, cand: np.ndarray, dist: np.ndarray, m: int, metric: int, alpha: float) -> np.ndarray:
    """table: padded [ntable, Dp] fp32 or fp16 (widened here: exact); cand int32 [n, K]; dist fp32 [n, K] internal.  -> uint8 [n, K]."""
    t32 = np.ascontiguousarray(table.astype(np.float32))
    cand = np.ascontiguousarray(cand, np.int32)
    dist = np.ascontiguousarray(dist, np.float32)
    n, K = cand.shape
    keep = np.full((n, K), 0xEE, np.uint8)
    rc = ref.lm_select_ref(t32.ctypes.data, t32.shape[0], t32.shape[1], metric, cand.ctypes.data, dist.ctypes.data, n, K, m, alpha, keep.ctypes.data)
    assert rc == 0, rc
    return keep


def internal_dist(x: np.ndarray, base: np.ndarray, cand: np.ndarray, metric: int) -> np.ndarray:
    """fp32 internal distance (squared L2 / -ip) of x[base[r]] to x[cand[r, j]]; slots whose id is out of range get +inf."""
    ok = (cand >= 0) & (cand < x.shape[0])
    v = x[np.where(ok, cand, 0)].astype(np.float32)
    b = x[base].astype(np.float32)[:, None, :]
    d = ((v - b) ** 2).sum(-1, dtype=np.float32) if metric == 1 else -(v * b).sum(-1, dtype=np.float32)
    return np.where(ok, d, np.float32(np.inf)).astype(np.float32)


def awkward_rows(x: np.ndarray, n: int, K: int, metric: int, seed: int):
    """n candidate rows over the table x, sorted best first, with: empty slots (-1) in the middle and at the tail, ids >= ntable (empty
    as well), duplicate ids inside a row, and -- when x holds duplicate vectors -- exact ties.  Returns (cand int32 [n, K], dist fp32)."""
    rng = np.random.default_rng(seed)
    N = x.shape[0]
    base = rng.integers(0, N, n)
    cand = np.stack([rng.permutation(N)[:K] if N >= K else rng.integers(0, N, K) for _ in range(n)]).astype(np.int32)
    if K >= 4:  # duplicate ids inside a row
        rows = rng.random(n) < 0.5
        cand[rows, K // 2] = cand[rows, 1]
    dist = internal_dist(x, base, cand, metric)
    o = np.argsort(dist, axis=1, kind="stable")
    cand, dist = np.take_along_axis(cand, o, 1), np.take_along_axis(dist, o, 1)
    tail = np.arange(K)[None, :] >= rng.integers(0, K + 1, n)[:, None]
    tail[rng.random(n) < 0.5] = False  # half of the rows are full
    mid = rng.random((n, K)) < 0.05
    cand[tail | mid] = -1
    over = (rng.random((n, K)) < 0.03) & ~(tail | mid)
    cand[over] = N + rng.integers(0, 5, int(over.sum())).astype(np.int32)  # ids >= ntable keep their (finite) distance: the id alone marks the slot empty
    dist[tail | mid] = np.float32(np.inf)
    return np.ascontiguousarray(cand), np.ascontiguousarray(dist)
