"""Helpers shared by the link-insertion tests (tests/test_link_kernel.py on the CPU, tests/test_gpu_link_kernel.py on the MI355X): compile
tests/link_ref/lm_link_ref.c -- the CPU restatement of lm_graph_add_links -- together with the unchanged tests/select_ref/lm_select_ref.c
against the oracle library, call it on numpy arrays, and generate a level graph plus an edge set with every awkward feature the contract
names."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
ORACLE_LIB = ROOT / "oracle" / "_build" / "liblm_oracle.so"


def compile_ref(out_dir: Path) -> Path:
    """As tests/select_ref_util.compile_ref: gcc -O2 -ffp-contract=off, linked against the already built oracle (orc_dist)."""
    out = Path(out_dir) / "liblm_link_ref.so"
    subprocess.run(["gcc", "-std=c11", "-O2", "-ffp-contract=off", "-fopenmp", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror", "-o", str(out),
                    str(ROOT / "tests" / "link_ref" / "lm_link_ref.c"), str(ROOT / "tests" / "select_ref" / "lm_select_ref.c"),
                    f"-L{ORACLE_LIB.parent}", "-llm_oracle", "-lm", f"-Wl,-rpath,{ORACLE_LIB.parent}"], check=True, capture_output=True)
    return out


def load_ref(path):
    lib = C.CDLL(str(path))
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    lib.lm_link_ref.argtypes = [vp, i32, i32, vp, vp, vp, i64, i32, vp, vp, vp, i64, C.c_float]
    lib.lm_link_ref.restype = C.c_int
    lib.lm_link_ref_pair_dists.argtypes = [vp, i32, i32, vp, vp, i64, vp]
    lib.lm_link_ref_pair_dists.restype = None
    return lib


def ref_link(ref, table: np.ndarray, adj: np.ndarray, dist: np.ndarray, deg: np.ndarray, src, dst, w, metric: int, alpha: float):
    """The restatement on COPIES of adj int32 [n, cap] / dist fp32 [n, cap] / deg int32 [n]; table: padded fp32 or fp16 (widened here:
    exact).  -> (adj, dist, deg) after the call."""
    t32 = np.ascontiguousarray(table.astype(np.float32))
    adj, dist, deg = np.array(adj, np.int32, order="C"), np.array(dist, np.float32, order="C"), np.array(deg, np.int32, order="C")
    src, dst, w = np.ascontiguousarray(src, np.int32), np.ascontiguousarray(dst, np.int32), np.ascontiguousarray(w, np.float32)
    n, cap = adj.shape
    rc = ref.lm_link_ref(t32.ctypes.data, t32.shape[1], metric, adj.ctypes.data, dist.ctypes.data, deg.ctypes.data, n, cap, src.ctypes.data, dst.ctypes.data,
                         w.ctypes.data, src.shape[0], alpha)
    assert rc == 0, rc
    return adj, dist, deg


def pair_dists(ref, table: np.ndarray, src: np.ndarray, dst: np.ndarray, metric: int) -> np.ndarray:
    """The canonical internal distance (orc_dist) of table[src[e]] and table[dst[e]]; ids must be in range."""
    t32 = np.ascontiguousarray(table.astype(np.float32))
    src, dst = np.ascontiguousarray(src, np.int32), np.ascontiguousarray(dst, np.int32)
    out = np.empty(src.shape[0], np.float32)
    ref.lm_link_ref_pair_dists(t32.ctypes.data, t32.shape[1], metric, src.ctypes.data, dst.ctypes.data, src.shape[0], out.ctypes.data)
    return out


def same_bytes(a, b) -> bool:
    """(adj, dist, deg) triples equal byte for byte (distances as bit patterns: a NaN equals the same NaN, -0 differs from +0)."""
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def edge_case_inputs(ref, table: np.ndarray, cap: int, metric: int, seed: int, stage: int):
    """A level graph over the n rows of ``table`` and an edge set that contains, by construction:
      * rows with no incoming edge (``untouched``), filled with a byte pattern -- ids, distances and degrees no call would write;
      * rows that end with fewer than cap (cap > 1), exactly cap, cap + 1 and more than 2 cap distinct candidates;
      * one row (``hub``) with at least 3 * stage incoming edges;
      * an incoming edge that repeats an existing link with a smaller weight; the same (src, dst) twice with different weights;
      * self edges, negative and >= n ids in src and in dst; existing rows with holes (-1, ids >= n, negative ids);
      * NaN and -0.0 weights; d_deg pre-filled with garbage.
    Needs n >= 2 cap + 40.  Returns a dict: adj, dist, deg, src, dst, w, untouched, hub, designed (row -> distinct candidates)."""
    rng = np.random.default_rng(seed)
    n = table.shape[0]
    assert n >= 2 * cap + 40
    t32 = table.astype(np.float32)
    adj = np.full((n, cap), -1, np.int32)
    dist = np.full((n, cap), np.inf, np.float32)
    deg = rng.integers(-5, 1 << 20, n).astype(np.int32)  # garbage: output only
    untouched = np.arange(n - 12, n)  # never a src
    rows = np.arange(n - 12)
    special = {"few": 0, "exact": 1, "plus1": 2, "many": 3, "hub": 4, "dup_existing": 5, "dup_pair": 6, "awkward_w": 7}
    # ---- existing lists of the ordinary rows: 0 .. cap entries, holes, a repeated id now and then
    for v in rows[8:]:
        k = int(rng.integers(0, cap + 1))
        ids = rng.permutation(n)[:k].astype(np.int32)
        ids = ids[ids != v]
        slots = np.sort(rng.permutation(cap)[: ids.shape[0]])  # holes between them
        adj[v, slots] = ids
        if ids.shape[0] >= 2 and rng.random() < 0.2:
            adj[v, slots[-1]] = ids[0]  # the same id in two slots: the first slot wins
        hole = np.setdiff1d(np.arange(cap), slots)
        if hole.shape[0]:
            adj[v, hole] = rng.choice(np.array([-1, -7, n, n + 3, np.iinfo(np.int32).max, np.iinfo(np.int32).min], np.int64), hole.shape[0]).astype(np.int32)
    ok = (adj >= 0) & (adj < n)
    vv, cc = np.nonzero(ok)
    dist[vv, cc] = pair_dists(ref, t32, vv.astype(np.int32), adj[vv, cc], metric)
    dist[~ok] = rng.choice(np.array([np.inf, 0.25, -3.0, np.nan], np.float32), int((~ok).sum()))  # whatever an empty slot holds is ignored
    # ---- untouched rows: a pattern that nothing the call writes would produce
    adj[untouched] = rng.integers(-(1 << 31), 1 << 31, (12, cap)).astype(np.int32)
    dist[untouched] = rng.integers(0, 1 << 32, (12, cap)).astype(np.uint32).view(np.float32)
    deg[untouched] = 0x5A5A5A5A
    src, dst, w = [], [], []

    def add(s, d, ww=None):
        s, d = np.atleast_1d(np.asarray(s, np.int32)), np.atleast_1d(np.asarray(d, np.int32))
        s = np.broadcast_to(s, d.shape).copy()
        inr = (s >= 0) & (s < n) & (d >= 0) & (d < n)
        x = np.zeros(d.shape[0], np.float32)
        x[inr] = pair_dists(ref, t32, s[inr], d[inr], metric)
        if ww is not None:
            x = np.broadcast_to(np.asarray(ww, np.float32), d.shape).copy()
        src.append(s), dst.append(d), w.append(x)

    def others(v, k):  # k distinct ids != v
        p = rng.permutation(n)
        return p[p != v][:k].astype(np.int32)

    designed = {}
    # rows whose candidate count is fixed: existing entries e, incoming distinct new ones the rest
    for name, total in (("few", max(cap - 1, 1)), ("exact", cap), ("plus1", cap + 1), ("many", 2 * cap + 9)):
        v = special[name]
        ids = others(v, total)
        e = int(rng.integers(0, min(cap, total - 1) + 1))  # at least one incoming edge
        adj[v, :] = -1
        dist[v, :] = np.inf
        adj[v, :e] = ids[:e]
        dist[v, :e] = pair_dists(ref, t32, np.full(e, v, np.int32), ids[:e], metric)
        add(v, ids[e:])
        add(v, ids[: max(1, e // 2)])  # and some that are there already
        designed[v] = total
    # the hub: >= 3 * stage incoming edges, every dst many times with different weights, spread over the whole edge array
    hub = special["hub"]
    hd = rng.integers(0, n, 3 * stage + 57).astype(np.int32)
    add(hub, hd, pair_dists(ref, t32, np.full(hd.shape[0], hub, np.int32), hd, metric) + rng.choice(np.array([0, 0, 0.125, -0.25], np.float32), hd.shape[0]))
    # an incoming edge repeats an existing link with a smaller weight: the existing weight survives
    v = special["dup_existing"]
    ids = others(v, min(cap, 3))
    adj[v, :] = -1
    dist[v, :] = np.inf
    adj[v, : ids.shape[0]] = ids
    dist[v, : ids.shape[0]] = pair_dists(ref, t32, np.full(ids.shape[0], v, np.int32), ids, metric)
    add(v, ids, dist[v, : ids.shape[0]] - 1.0)
    # the same (src, dst) twice among the edges, different weights: the lower index wins (here the LARGER weight comes first)
    v = special["dup_pair"]
    ids = others(v, 5)
    add(v, ids, 0.5)
    add(v, ids, -0.5)
    # NaN and -0.0 weights (and +0.0 beside -0.0: a tie that goes to the lower dst)
    v = special["awkward_w"]
    ids = others(v, 6)
    add(v, ids, np.array([np.nan, -0.0, 0.0, -0.0, np.nan, 0.0], np.float32))
    # ordinary traffic: every ordinary row a few times, some rows a lot
    s = rng.choice(rows[8:], 6 * n)
    add(s, rng.integers(0, n, s.shape[0]))
    s = rng.choice(rows[8:40], 4 * cap * 8)
    add(s, rng.integers(0, n, s.shape[0]))
    # invalid edges: self edges, ids out of range on either side (some name an untouched row as src: still not affected)
    bad_s = np.concatenate([rows[:30], [-1, -9, n, n + 5, np.iinfo(np.int32).max], untouched[:4], untouched[4:8], rows[8:12]]).astype(np.int64)
    bad_d = np.concatenate([rows[:30], rows[:5], untouched[:4], [-1, n, -3, n + 1], [-2, n, np.iinfo(np.int32).min, np.iinfo(np.int32).max]]).astype(np.int64)
    add(bad_s.astype(np.int32), bad_d.astype(np.int32), rng.standard_normal(bad_s.shape[0]).astype(np.float32))
    src, dst, w = np.concatenate(src), np.concatenate(dst), np.concatenate(w)
    o = order_preserving_permutation(src, dst, rng)  # mix the groups: a row's edges are not contiguous
    out = dict(adj=adj, dist=dist, deg=deg, src=np.ascontiguousarray(src[o]), dst=np.ascontiguousarray(dst[o]), w=np.ascontiguousarray(w[o]), untouched=untouched, hub=hub,
               designed=designed)
    valid = (out["src"] >= 0) & (out["src"] < n) & (out["dst"] >= 0) & (out["dst"] < n) & (out["src"] != out["dst"])
    assert int((valid & (out["src"] == hub)).sum()) >= 3 * stage  # (57 to spare: a few of the hub's random dsts are the hub itself)
    assert not np.isin(out["src"][valid], untouched).any()
    return out


def order_preserving_permutation(src: np.ndarray, dst: np.ndarray, rng) -> np.ndarray:
    """A random order of the edges in which every two edges with the same (src, dst) keep their relative order."""
    ne = src.shape[0]
    r = rng.permutation(ne)
    g = src.astype(np.int64) * (1 << 32) + (dst.astype(np.int64) & 0xFFFFFFFF)
    by_e = np.lexsort((np.arange(ne), g))  # groups, members by edge index
    by_r = np.lexsort((r, g))  # groups, members by random key
    rr = np.empty(ne, np.int64)
    rr[by_e] = r[by_r]  # the group's random keys, handed out in ascending order to its members in edge order
    return np.argsort(rr, kind="stable")
