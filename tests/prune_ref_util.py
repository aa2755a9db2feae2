"""Helpers shared by the hub-preserving pruning tests (tests/test_prune_kernel.py on the CPU, tests/test_gpu_prune_kernel.py on the
MI355X): compile tests/prune_ref/lm_prune_ref.c -- the CPU restatement of lm_graph_prune_hubs -- together with the unchanged
tests/link_ref/lm_link_ref.c and tests/select_ref/lm_select_ref.c against the oracle library, call it on numpy arrays, and generate
level-0 adjacencies and tables with every awkward feature the contract names."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
ORACLE_LIB = ROOT / "oracle" / "_build" / "liblm_oracle.so"


def compile_ref(out_dir: Path) -> Path:
    """As tests/link_ref_util.compile_ref: gcc -O2 -ffp-contract=off, linked against the already built oracle (orc_dist)."""
    out = Path(out_dir) / "liblm_prune_ref.so"
    subprocess.run(["gcc", "-std=c11", "-O2", "-ffp-contract=off", "-fopenmp", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror", "-o", str(out),
                    str(ROOT / "tests" / "prune_ref" / "lm_prune_ref.c"), str(ROOT / "tests" / "link_ref" / "lm_link_ref.c"),
                    str(ROOT / "tests" / "select_ref" / "lm_select_ref.c"), f"-L{ORACLE_LIB.parent}", "-llm_oracle", "-lm", f"-Wl,-rpath,{ORACLE_LIB.parent}"],
                   check=True, capture_output=True)
    return out


def load_ref(path):
    lib = C.CDLL(str(path))
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    lib.lm_prune_ref.argtypes = [vp, i32, i32, vp, i64, i32, i32, i64, C.c_float, vp, vp, vp, vp, vp]
    lib.lm_prune_ref.restype = C.c_int
    return lib


def ref_prune(ref, table: np.ndarray, adj: np.ndarray, m_low: int, n_hubs: int, metric: int, alpha: float):
    """The restatement.  table: padded fp32 or fp16 (widened here: exact); adj int32 [n, cap].  -> (adj, dist, deg, hubs, indeg)."""
    t32 = np.ascontiguousarray(table.astype(np.float32))
    adj = np.ascontiguousarray(adj, np.int32)
    n, cap = adj.shape
    a, d, g = np.full((n, cap), 0x55555555, np.int32), np.full((n, cap), 3.25, np.float32), np.full(n, 0x55555555, np.int32)
    hubs, indeg = np.full(n_hubs, 0x55555555, np.int32), np.full(n, 0x55555555, np.int32)
    rc = ref.lm_prune_ref(t32.ctypes.data, t32.shape[1], metric, adj.ctypes.data, n, cap, m_low, n_hubs, alpha, a.ctypes.data, d.ctypes.data, g.ctypes.data,
                          hubs.ctypes.data, indeg.ctypes.data)
    assert rc == 0, rc
    return a, d, g, hubs, indeg


NAMES = ("adj", "dist", "deg", "hubs", "indeg")


def differing(a, b) -> list:
    """Names of the arrays of two (adj, dist, deg, hubs, indeg) results that are not equal byte for byte (distances as bit patterns)."""
    return [nm for nm, x, y in zip(NAMES, a, b) if not (x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes())]


def usable_mask(adj: np.ndarray) -> np.ndarray:
    n = adj.shape[0]
    return (adj >= 0) & (adj < n) & (adj != np.arange(n, dtype=np.int64)[:, None])


def in_degrees(adj: np.ndarray) -> np.ndarray:
    return np.bincount(adj[usable_mask(adj)].astype(np.int64), minlength=adj.shape[0]).astype(np.int32)


def tie_cut(adj: np.ndarray, row: int = 1024) -> int:
    """An n_hubs that cuts a group of nodes of EQUAL in-degree in its middle.  Where the graph has more than ``row`` nodes the group is
    one with members on both sides of node ``row`` (the scan's first tile boundary) and the cut falls right after its first member at or
    beyond ``row`` -- or right before it when that is the group's last member."""
    indeg = in_degrees(adj)
    n = adj.shape[0]
    best = None
    for T in np.unique(indeg):
        members = np.nonzero(indeg == T)[0]
        if members.shape[0] < 2:
            continue
        if n > row:
            if not (members[0] < row <= members[-1]):
                continue
            idx = int(np.searchsorted(members, row))  # >= 1 members lie below `row`
            kr = idx + 1 if idx + 1 < members.shape[0] else idx
        else:
            kr = members.shape[0] // 2
        if best is None or members.shape[0] > best[0]:
            best = (members.shape[0], int((indeg > T).sum()) + kr)
    assert best is not None, "no group of equal in-degrees to cut"
    return best[1]


def table_for(n: int, d: int, seed: int, f16: bool) -> np.ndarray:
    """A padded table with duplicated vectors (exact distance ties) and, from 16 rows on, a NaN row (3) and an all-zero row (4)."""
    from tests.select_ref_util import pad64
    from tests.util import clustered

    x = clustered(max(n, 8), d, seed, n_centers=8, sigma=0.5)[:n]
    nd = n // 6
    x[:nd] = x[nd : 2 * nd]
    if n >= 16:
        x[3] = np.nan
        x[4] = 0.0
    return pad64(x.astype(np.float16) if f16 else x)


JUNK = np.array([-1, -7, np.iinfo(np.int32).max, np.iinfo(np.int32).min], np.int64)


def edge_case_adj(n: int, cap: int, seed: int, stage: int = 0) -> np.ndarray:
    """A level-0 adjacency int32 [n, cap] with: rows of 0 .. cap entries with holes between them; hole values < 0 and >= n; self links; a
    neighbour listed twice; rows with fewer usable slots than any quota (empty rows among them); in-degrees with many ties; and, when
    ``stage`` > 0 (needs n >= 3 * stage + 100 and cap >= 2), a star: 3 * stage + 16 rows list node 7 in their first slot, so that row 7
    receives that many reverse edges."""
    rng = np.random.default_rng(seed)
    adj = np.full((n, cap), -1, np.int32)
    junk = np.concatenate([JUNK, [n, n + 3]])
    for v in range(n):
        k = int(rng.integers(0, cap + 1))
        if n == 1:
            ids = np.zeros(0, np.int64)
        else:
            ids = rng.integers(0, n, k)
        slots = np.sort(rng.permutation(cap)[: ids.shape[0]])
        adj[v, slots] = ids  # (some of them v itself: self links)
        if ids.shape[0] >= 2 and rng.random() < 0.25:
            adj[v, slots[-1]] = ids[0]  # the same neighbour twice
        hole = np.setdiff1d(np.arange(cap), slots)
        if hole.shape[0]:
            adj[v, hole] = rng.choice(junk, hole.shape[0]).astype(np.int32)
        if rng.random() < 0.05:
            adj[v, int(rng.integers(0, cap))] = v  # a self link for sure
    if n >= 40:
        adj[n // 3] = -1  # an empty row
        adj[n // 3 + 1] = n // 3 + 1  # nothing but self links
    if stage > 0:
        assert n >= 3 * stage + 100 and cap >= 2
        rows = rng.permutation(np.arange(8, n))[: 3 * stage + 16]
        adj[rows, 0] = 7
    return adj


def check_star(adj: np.ndarray, stage: int) -> int:
    """The in-degree of the star's centre; asserts that it is above 3 * stage."""
    c = int(in_degrees(adj)[7])
    assert c > 3 * stage, c
    return c


def hubs_of_kind(kind: str, adj: np.ndarray) -> int:
    n = adj.shape[0]
    return {"0": 0, "1": min(1, n), "n": n}[kind] if kind != "tie" else tie_cut(adj)


# The edge-case set both suites run (the emulation on the CPU, tests/test_gpu_prune_kernel.py its n = 3000 part on the MI355X): table
# seed 100 + i, graph seed 300 + i for entry i.  The star needs n = 3000.
# (n, cap, m_low, n_hubs kind, d, metric, f16, alpha, star, twice)
EDGE_RUNS = [
    (1, 1, 1, "0", 48, 0, False, 1.0, False, False),
    (1, 8, 3, "n", 48, 1, True, 1.2, False, False),
    (2, 1, 1, "1", 48, 1, False, 1.0, False, True),
    (2, 8, 13, "n", 384, 0, True, 1.0, False, False),
    (2, 64, 64, "0", 48, 0, False, 1.2, False, False),
    (1023, 8, 3, "tie", 48, 0, False, 1.0, False, False),
    (1023, 1, 6, "tie", 48, 1, True, 1.0, False, False),
    (1025, 8, 3, "tie", 384, 1, True, 1.2, False, True),
    (1025, 1, 1, "1", 48, 0, False, 1.2, False, False),
    (1025, 64, 3, "tie", 48, 1, False, 1.0, False, False),
    (1025, 8, 8, "0", 48, 0, True, 1.0, False, False),
    (3000, 8, 3, "tie", 48, 0, False, 1.0, True, True),
    (3000, 8, 3, "tie", 384, 1, True, 1.2, True, False),
    (3000, 8, 13, "n", 48, 1, False, 1.2, True, False),
    (3000, 8, 1, "1", 48, 0, True, 1.0, True, False),
    (3000, 64, 3, "tie", 48, 1, True, 1.0, True, False),
    (3000, 64, 69, "1", 48, 0, False, 1.2, True, False),
    (3000, 1, 1, "tie", 48, 1, False, 1.0, False, False),
]
