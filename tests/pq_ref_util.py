"""Helpers shared by the PQ build tests (tests/test_pq_build.py on the CPU, tests/test_gpu_pq_build.py on the MI355X): compile
tests/pq_ref/lm_pq_ref.c -- the CPU restatement of lm_pq_encode / lm_pq_train --, call it on numpy arrays, and the second pin of the
encoder's arithmetic: argmin over the oracle's orc_pq_lut table (the table the search reads)."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent


def compile_ref(out_dir: Path) -> Path:
    out = Path(out_dir) / "liblm_pq_ref.so"
    subprocess.run(["gcc", "-std=c11", "-O2", "-ffp-contract=off", "-fopenmp", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror", "-o", str(out),
                    str(ROOT / "tests" / "pq_ref" / "lm_pq_ref.c"), "-lm"], check=True, capture_output=True)
    return out


def load_ref(path):
    lib = C.CDLL(str(path))
    lib.lm_pq_ref_encode.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.lm_pq_ref_encode.restype = C.c_int
    lib.lm_pq_ref_train.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
    lib.lm_pq_ref_train.restype = C.c_int
    return lib


def _offsets(chunk_offsets):
    return None if chunk_offsets is None else np.ascontiguousarray(chunk_offsets, np.int32)


def n_chunks(codebooks: np.ndarray, chunk_offsets) -> int:
    return int(codebooks.shape[0]) if chunk_offsets is None else len(chunk_offsets) - 1


def ref_encode(ref, x: np.ndarray, d: int, codebooks: np.ndarray, chunk_offsets=None) -> np.ndarray:
    """x: [n, ld] fp32 or fp16 (widened here: exact), the first d columns are the vector.  codebooks: [m, 256, d/m] (uniform) or the flat
    chunked layout with chunk_offsets.  -> uint8 [n, m]."""
    x32 = np.ascontiguousarray(x.astype(np.float32))
    cb = np.ascontiguousarray(codebooks, np.float32)
    off = _offsets(chunk_offsets)
    m = n_chunks(cb, chunk_offsets)
    codes = np.full((x32.shape[0], m), 0xEE, np.uint8)
    rc = ref.lm_pq_ref_encode(x32.ctypes.data, x32.shape[0], x32.shape[1], d, m, None if off is None else off.ctypes.data, cb.ctypes.data, codes.ctypes.data)
    assert rc == 0, rc
    return codes


def ref_train(ref, x: np.ndarray, d: int, init: np.ndarray, iters: int, chunk_offsets=None) -> np.ndarray:
    """Lloyd iterations from the centroids `init` (same layout as ref_encode's codebooks); returns the trained copy."""
    x32 = np.ascontiguousarray(x.astype(np.float32))
    cb = np.array(init, np.float32, order="C", copy=True)
    off = _offsets(chunk_offsets)
    m = n_chunks(cb, chunk_offsets)
    rc = ref.lm_pq_ref_train(x32.ctypes.data, x32.shape[0], x32.shape[1], d, m, None if off is None else off.ctypes.data, iters, cb.ctypes.data)
    assert rc == 0, rc
    return cb


def lut_argmin_codes(x: np.ndarray, d: int, codebooks: np.ndarray, chunk_offsets=None) -> np.ndarray:
    """The codes from the oracle's side: for every row, orc_pq_lut(row as the query, L2) -> [m, 256]; code = the first minimum of each row of
    the table, a NaN entry never being one (all NaN: 0)."""
    from oracle import oracle as orc

    x32 = np.ascontiguousarray(x.astype(np.float32))
    cb = np.ascontiguousarray(codebooks, np.float32)
    m = n_chunks(cb, chunk_offsets)
    if x32.shape[1] < 1:
        x32 = np.zeros((x32.shape[0], 1), np.float32)
    dummy = np.zeros((1, m), np.uint8)
    pq, _keep, _ = orc._pq_struct(cb, dummy, chunk_offsets)
    out = np.zeros((x32.shape[0], m), np.uint8)
    lut = np.empty((m, 256), np.float32)
    for v in range(x32.shape[0]):
        row = np.ascontiguousarray(x32[v])
        orc.lib().orc_pq_lut(C.byref(pq), row.ctypes.data_as(C.c_void_p), 1, lut.ctypes.data_as(C.c_void_p))
        out[v] = np.where(np.isnan(lut), np.float32(np.inf), lut).argmin(1)
    return out


def recon_mse(x: np.ndarray, codebooks: np.ndarray, codes: np.ndarray) -> float:
    """Mean squared reconstruction error (float64) of uniform codebooks [m, 256, dsub] over x [n, d]."""
    m, _, dsub = codebooks.shape
    rec = codebooks[np.arange(m)[None, :], codes.astype(np.int64)].reshape(x.shape[0], m * dsub)
    return float(((x.astype(np.float64) - rec.astype(np.float64)) ** 2).sum(1).mean())
