"""Helpers shared by the insert-step tests (tests/test_insert_kernel.py on the CPU, tests/test_gpu_insert_kernel.py on the MI355X): compile
tests/insert_ref/lm_insert_ref.c -- the CPU restatement of lm_graph_insert_batch -- together with the unchanged
tests/select_ref/lm_select_ref.c and tests/link_ref/lm_link_ref.c against the oracle library, build the layered test graph, and run one
call of the library against the restatement: candidates, candidate distances (as bit patterns), keep masks and the three level arrays
byte for byte, the search statistics equal to those of the separate search that supplies S."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
ORACLE_LIB = ROOT / "oracle" / "_build" / "liblm_oracle.so"
STAT_KEYS = ("ndis", "nexpand", "nrounds")
N, ROWS, CAPS = 2000, (2000, 130, 9), (16, 8, 8)
FILL_I32, FILL_F32, FILL_U8 = 0x6E6E6E6E, 7.5, 0x6E


def compile_ref(out_dir: Path) -> Path:
    """As tests/link_ref_util.compile_ref: gcc -O2 -ffp-contract=off, linked against the already built oracle (orc_dist)."""
    out = Path(out_dir) / "liblm_insert_ref.so"
    subprocess.run(["gcc", "-std=c11", "-O2", "-ffp-contract=off", "-fopenmp", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror", "-o", str(out),
                    str(ROOT / "tests" / "insert_ref" / "lm_insert_ref.c"), str(ROOT / "tests" / "link_ref" / "lm_link_ref.c"),
                    str(ROOT / "tests" / "select_ref" / "lm_select_ref.c"), f"-L{ORACLE_LIB.parent}", "-llm_oracle", "-lm", f"-Wl,-rpath,{ORACLE_LIB.parent}"],
                   check=True, capture_output=True)
    return out


def load_ref(path):
    lib = C.CDLL(str(path))
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    lib.lm_insert_ref_queries.argtypes = [vp, i32, i32, i64, vp, i64, vp]
    lib.lm_insert_ref_queries.restype = None
    lib.lm_insert_ref.argtypes = [vp, i32, i32, i64, i32, vp, i64, i32, i32, i32, C.c_float, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.lm_insert_ref.restype = C.c_int
    return lib


def ref_queries(ref, table: np.ndarray, d: int, batch: np.ndarray) -> np.ndarray:
    """Step 1.  table: padded fp32 or fp16 (widened here: exact)."""
    t32 = np.ascontiguousarray(table.astype(np.float32))
    batch = np.ascontiguousarray(batch, np.int32)
    q = np.full((batch.shape[0], d), np.nan, np.float32)
    ref.lm_insert_ref_queries(t32.ctypes.data, t32.shape[1], d, t32.shape[0], batch.ctypes.data, batch.shape[0], q.ctypes.data)
    return q


def ref_insert(ref, table: np.ndarray, metric: int, adj, dist, deg, batch, replace: bool, kk: int, m: int, alpha: float, s_labels, s_dist):
    """Steps 3-9 on COPIES of the level arrays.  -> (cand, cdist, keep, adj, dist, deg)."""
    t32 = np.ascontiguousarray(table.astype(np.float32))
    adj, dist, deg = np.array(adj, np.int32, order="C"), np.array(dist, np.float32, order="C"), np.array(deg, np.int32, order="C")
    batch = np.ascontiguousarray(batch, np.int32)
    s_labels, s_dist = np.ascontiguousarray(s_labels, np.int64), np.ascontiguousarray(s_dist, np.float32)
    n, cap = adj.shape
    b = batch.shape[0]
    K = kk + (cap if replace else 0)
    cand, cdist, keep = np.full((b, K), 0x55555555, np.int32), np.full((b, K), 3.25, np.float32), np.full((b, K), 0x55, np.uint8)
    rc = ref.lm_insert_ref(t32.ctypes.data, t32.shape[1], metric, n, cap, batch.ctypes.data, b, 1 if replace else 0, kk, m, alpha, s_labels.ctypes.data,
                           s_dist.ctypes.data, adj.ctypes.data, dist.ctypes.data, deg.ctypes.data, cand.ctypes.data, cdist.ctypes.data, keep.ctypes.data)
    assert rc == 0, rc
    return cand, cdist, keep, adj, dist, deg


NAMES = ("cand", "cdist", "keep", "adj", "dist", "deg")


def differing(a, b) -> list:
    """Names of the arrays of two (cand, cdist, keep, adj, dist, deg) results that are not equal byte for byte (distances as bit patterns)."""
    return [nm for nm, x, y in zip(NAMES, a, b) if not (x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes())]


_GRAPHS = {}


def layered_graph(d: int, metric: int):
    """(x, levels, entry, marks): 2000 clustered points on three nested levels of 2000 / 130 / 9 rows with caps 16 / 8 / 8; a row links its
    node to its nearest nodes of the level (3 .. cap - 4 of them, so that rows keep room), scattered over the slots with holes in between;
    one row per level filled to cap, one emptied, one slot holding an out-of-range value.  marks = the level-0 rows (full, empty, the one
    with the out-of-range slot)."""
    from tests.util import clustered

    key = (d, metric)
    if key in _GRAPHS:
        return _GRAPHS[key]
    rng = np.random.default_rng(100 + d + metric)
    x = clustered(N, d, 7 + d, n_centers=16, sigma=0.6)
    sim = x @ x.T  # unit vectors: the nearest by inner product are the nearest by L2
    np.fill_diagonal(sim, -np.inf)
    order = rng.permutation(N)
    levels, marks = [], None
    for l, (rows, cap) in enumerate(zip(ROWS, CAPS)):
        ids = np.sort(order[:rows]).astype(np.int32)
        adj = np.full((rows, cap), -1, np.int32)
        for r, v in enumerate(ids):
            m = int(rng.integers(3, cap - 3))
            nb = ids[np.argsort(-sim[v, ids], kind="stable")[:m]]
            adj[r, np.sort(rng.permutation(cap)[:m])] = nb
        full, empty = [int(r) for r in rng.permutation(rows) if ids[r] != order[0]][:2]  # (the entry point keeps its row)
        adj[full] = ids[np.argsort(-sim[ids[full], ids], kind="stable")[:cap]]
        adj[empty] = -1
        hole = tuple(np.argwhere(adj == -1)[0])
        adj[hole] = N + 3
        if l == 0:
            marks = (full, empty, int(hole[0]))
        levels.append((None if l == 0 else ids, adj))
    _GRAPHS[key] = (x, levels, int(order[0]), marks)
    return _GRAPHS[key]


def level0_arrays(x: np.ndarray, adj: np.ndarray, metric: int):
    """(dist fp32 [n, cap], deg int32 [n]) beside a level-0 adjacency: the internal distance of every valid slot (fp32 arithmetic; to the
    call these are given bits), +inf elsewhere."""
    n, cap = adj.shape
    ok = (adj >= 0) & (adj < n)
    u = np.where(ok, adj, 0)
    xv = x.astype(np.float32)
    if metric == 1:
        dd = ((xv[:, None, :] - xv[u]) ** 2).sum(-1, dtype=np.float32)
    else:
        dd = -(xv[:, None, :] * xv[u]).sum(-1, dtype=np.float32)
    return np.where(ok, dd, np.float32(np.inf)).astype(np.float32), ok.sum(1).astype(np.int32)


class Level:
    """One view index over copies of the level arrays, where the library's kernels run: host tensors for the host build of the library
    (``device`` None), else tensors on the torch device."""

    def __init__(self, x: np.ndarray, levels, entry: int, metric: int, f16: bool, device=None, attach: bool = True):
        import torch

        from leann_amd.index import Mi355xIndex
        from tests.select_ref_util import pad64
        from tests.view_ref_util import as_tensors

        self.n, self.d = x.shape
        self.metric, self.device = metric, device
        with np.errstate(all="ignore"):  # (the overflow case stores 3e38: inf as fp16, inf / NaN distances)
            self.table = pad64(x.astype(np.float16) if f16 else x.astype(np.float32))
            d0, g0 = level0_arrays(self.table[:, : self.d].astype(np.float32), levels[0][1], metric)
        lt = as_tensors([(nd, a.copy()) for nd, a in levels], device)  # copies: the call writes into level 0
        self.adj = lt[0][1]
        self.dist = torch.from_numpy(np.ascontiguousarray(d0))
        self.deg = torch.from_numpy(np.ascontiguousarray(g0))
        if device is not None:
            self.dist, self.deg = self.dist.to(device), self.deg.to(device)
        self.idx = Mi355xIndex.from_levels(lt, self.n, self.d, metric, entry)
        if attach:
            if device is None:
                self.idx.attach_table(self.table[:, : self.d])
            else:
                self.idx.set_stream(torch.cuda.current_stream(device).cuda_stream)
                self._tab = torch.from_numpy(self.table).to(device)
                self.idx.attach_table(self._tab)

    def arrays(self):
        return self.adj.cpu().numpy().copy(), self.dist.cpu().numpy().copy(), self.deg.cpu().numpy().copy()

    def tensor(self, a: np.ndarray):
        import torch

        t = torch.from_numpy(np.ascontiguousarray(a))
        return t if self.device is None else t.to(self.device)

    def stats(self):
        st = self.idx.stats()
        return {f: int(st[f]) for f in STAT_KEYS}

    def search(self, q: np.ndarray, k: int, prm):
        """lm_index_search_device on the view (host pointers on the host build).  -> (dist, labels) numpy."""
        import torch

        from leann_amd import _lib

        qt = self.tensor(q.astype(np.float32))
        n = qt.shape[0]
        dist = torch.empty((n, k), dtype=torch.float32, device=qt.device)
        ids = torch.empty((n, k), dtype=torch.int64, device=qt.device)
        _lib.check(self.idx._lib.lm_index_search_device(self.idx._h, n, C.c_void_p(qt.data_ptr()), k, C.c_void_p(dist.data_ptr()), C.c_void_p(ids.data_ptr()),
                                                       C.byref(prm)), "lm_index_search_device")
        return dist.cpu().numpy(), ids.cpu().numpy()

    def close(self):
        self.idx.close()


def run_insert(ref, L: Level, batch: np.ndarray, replace: bool, kk: int, m: int, alpha: float, ef: int, beam: int = 2, outputs: bool = True):
    """One lm_graph_insert_batch call on ``L`` against the restatement.  S comes from the separate view search on the queries of step 1,
    made before the call.  -> dict(diff=names of differing arrays, got, exp, S=(dist, labels), stats_equal, internal=internal distances of S)."""
    batch = np.ascontiguousarray(batch, np.int32)
    prm = L.idx.make_params(ef=ef, beam=beam, recompute=False, max_batch=16384)
    q = ref_queries(ref, L.table, L.d, batch)
    sd, sl = L.search(q, kk, prm)
    st_search = L.stats()
    a0, d0, g0 = L.arrays()
    exp = ref_insert(ref, L.table, L.metric, a0, d0, g0, batch, replace, kk, m, alpha, sl, sd)
    outs = L.idx.insert_batch(L.tensor(batch), replace, kk, m, alpha, prm, L.adj, L.dist, L.deg, return_candidates=outputs)
    st_insert = L.stats()
    a1, d1, g1 = L.arrays()
    if outputs:
        got = tuple(t.cpu().numpy() for t in outs) + (a1, d1, g1)
        diff = differing(got, exp)
    else:
        got = exp[:3] + (a1, d1, g1)
        diff = differing(got, exp)
    return dict(diff=diff, got=got, exp=exp, S=(sd, sl), stats_equal=st_search == st_insert, stats=st_insert, internal=sd if L.metric == 1 else -sd,
                before=(a0, d0, g0))


def emptied(levels, x: np.ndarray, metric: int, count: int, seed: int):
    """Level arrays in which ``count`` level-0-only nodes have empty rows and nobody links to them: (levels, ids)."""
    rng = np.random.default_rng(seed)
    n = levels[0][1].shape[0]
    upper = np.zeros(n, bool)
    upper[levels[1][0]] = True
    ids = np.sort(rng.permutation(np.nonzero(~upper)[0])[:count]).astype(np.int32)
    adj = levels[0][1].copy()
    gone = np.zeros(n, bool)
    gone[ids] = True
    adj[ids] = -1
    inr = (adj >= 0) & (adj < n)
    adj[inr & gone[np.where(inr, adj, 0)]] = -1
    out = [(None, adj)] + [(nd, a.copy()) for nd, a in levels[1:]]
    return out, ids


# ------------------------------------------------------------------------------------------------------------------------------------
# The edge-case set both suites run (tests/emulated_insert_cases.py on the host build of the library, tests/test_gpu_insert_kernel.py on
# the MI355X): every function takes (ref, device, d, metric, f16), asserts, and returns a line for the log.
# ------------------------------------------------------------------------------------------------------------------------------------
def _contract_checks(r, L: Level, batch, replace, kk, m):
    """What the header says about the result, independent of either implementation."""
    cand, cdist, keep, adj, dist, deg = r["got"]
    n = L.n
    live = (batch >= 0) & (batch < n)
    empty = cand < 0
    assert ((cand >= 0) & (cand < n) | (cand == -1)).all() and np.isinf(cdist[empty]).all() and (cdist[empty] > 0).all() and np.isfinite(cdist[~empty]).all()
    assert empty[~live].all() and not keep[~live].any() and not keep[empty].any() and (keep.sum(1) <= m).all()
    if replace:
        for i in np.nonzero(live)[0]:
            c = cand[i][cand[i] >= 0]
            assert np.unique(c).shape[0] == c.shape[0] and batch[i] not in c  # no id twice, not the node itself (no row of these graphs lists itself)
            dd = cdist[i][cand[i] >= 0]
            assert (np.diff(dd) >= 0).all() and (cand[i][c.shape[0]:] == -1).all()  # ordered, empties last
    valid = (adj >= 0) & (adj < n)
    assert np.array_equal(valid.sum(1), deg)
    touched = np.zeros(n, bool)
    touched[batch[live]] = True
    kept_ids = cand[keep.astype(bool)]
    touched[kept_ids] = True
    a0, d0, g0 = r["before"]
    assert adj[~touched].tobytes() == a0[~touched].tobytes() and dist[~touched].tobytes() == d0[~touched].tobytes() and np.array_equal(deg[~touched], g0[~touched])


def _finish(r, tag):
    assert not r["diff"], (tag, r["diff"])
    assert r["stats_equal"] and r["stats"]["ndis"] > 0, (tag, r["stats"])
    return f"{tag}: kept {int(r['got'][2].sum())} of {int((r['got'][0] >= 0).sum())} candidates, ndis={r['stats']['ndis']}: ok"


def case_insert_300(ref, device, d, metric, f16):
    """replace = 0: 300 rows are emptied first and nobody links to them; they are inserted as one batch with kk = 12, m = 8."""
    x, levels, entry, _ = layered_graph(d, metric)
    lv, ids = emptied(levels, x, metric, 300, 5)
    L = Level(x, lv, entry, metric, f16, device)
    a0 = L.arrays()[0]
    assert (a0[ids] == -1).all() and not np.isin(a0, ids).any()
    r = run_insert(ref, L, ids, False, 12, 8, 1.0, 40)
    _contract_checks(r, L, ids, False, 12, 8)
    assert not np.isin(r["S"][1], ids).any() and (r["got"][5][ids] > 0).all()  # the search cannot find them; afterwards each has links
    assert np.isin(r["got"][3], ids).any()  # ... and some rows link back
    L.close()
    return _finish(r, "insert 300")


def case_refine_257(ref, device, d, metric, f16):
    """replace = 1, b = 257 with the entry point's row, the full row, the empty row and the row with the out-of-range slot: K = 13 + 16 = 29
    (no multiple of 64), then K = 70 + 16 = 86 (two 64-slot pieces) on the same handle."""
    x, levels, entry, marks = layered_graph(d, metric)
    out = []
    L = Level(x, levels, entry, metric, f16, device)
    for kk, ef in ((13, 40), (70, 70)):
        rng = np.random.default_rng(kk)
        special = np.array([entry, *marks], np.int64)
        rest = rng.permutation(np.setdiff1d(np.arange(N), special))[: 257 - special.shape[0]]
        batch = rng.permutation(np.concatenate([special, rest])).astype(np.int32)
        assert batch.shape[0] == 257 and kk + 16 in (29, 86)
        r = run_insert(ref, L, batch, True, kk, 8, 1.0, ef)
        _contract_checks(r, L, batch, True, kk, 8)
        out.append(_finish(r, f"refine 257 K={kk + 16}"))
    L.close()
    return "; ".join(out)


def with_long_links(levels, marks):
    """The fixture links nearest neighbours only, so a walk stays inside a cluster of ~100 nodes.  Two random long links per level-0 row
    (in free slots; the marked rows stay as they are) make the level one component."""
    rng = np.random.default_rng(31)
    adj = levels[0][1].copy()
    for v in range(N):
        free = np.nonzero(adj[v] == -1)[0]
        if v in marks or free.shape[0] < 2:
            continue
        far = rng.permutation(np.setdiff1d(np.arange(N), np.append(adj[v], v)))[:2]
        adj[v, free[:2]] = far
    return [(None, adj)] + list(levels[1:])


def case_refine_k512(ref, device, d, metric, f16):
    """replace = 1, b = 8, kk = 496 at efSearch 496: K = 512, the mask's last word and the largest LDS image."""
    x, levels, entry, marks = layered_graph(d, metric)
    levels = with_long_links(levels, marks)  # (so that the search fills all 496 places)
    L = Level(x, levels, entry, metric, f16, device)
    batch = np.array([entry, *marks, 11, 500, 1234, 1999], np.int32)
    r = run_insert(ref, L, batch, True, 496, 8, 1.0, 496)
    _contract_checks(r, L, batch, True, 496, 8)
    assert (r["S"][1] >= 0).all(1).any() and r["got"][0].shape == (8, 512) and (r["got"][0][:, 448:] >= 0).any()  # candidates reach the last word
    L.close()
    return _finish(r, "refine K=512")


def case_twin_rows(ref, device, d, metric, f16):
    """Two identical table rows: their distances to any query are equal, so the position decides; every refinement row dedupes search
    entries against its own stored slots and drops itself.  Both events are asserted on the inputs."""
    x, levels, entry, marks = layered_graph(d, metric)
    levels = with_long_links(levels, marks)
    x = x.copy()
    adj0 = levels[0][1]
    a = entry  # (the walk starts there: its neighbourhood is found whatever the upper levels do)
    nb = adj0[a][(adj0[a] >= 0) & (adj0[a] < N)]
    t = int(nb[0])
    x[t] = x[a]  # node t becomes a's twin (it stays a's neighbour)
    L = Level(x, levels, entry, metric, f16, device)
    batch = np.unique(np.concatenate([[a, t], nb, adj0[t][(adj0[t] >= 0) & (adj0[t] < N)]])).astype(np.int32)
    r = run_insert(ref, L, batch, True, 20, 8, 1.0, 40)
    _contract_checks(r, L, batch, True, 20, 8)
    sd, sl = r["S"]
    before = r["before"][0]
    ties = dedupes = selfs = 0
    for i, v in enumerate(batch):
        ia, it = np.nonzero(sl[i] == a)[0], np.nonzero(sl[i] == t)[0]
        if ia.size and it.size and v not in (a, t):
            assert sd[i, ia[0]].tobytes() == sd[i, it[0]].tobytes()  # equal bits
            ca, ct = np.nonzero(r["got"][0][i] == a)[0], np.nonzero(r["got"][0][i] == t)[0]
            assert ca.size and ct.size and (ca[0] < ct[0]) == (ia[0] < it[0])  # the order of their positions survives
            ties += 1
        row = before[v][(before[v] >= 0) & (before[v] < N)]
        dedupes += int(np.isin(row, sl[i]).any())
        selfs += int((sl[i] == v).any())
    assert ties > 0 and dedupes > 0 and selfs > 0, (ties, dedupes, selfs, batch.shape[0])
    L.close()
    return _finish(r, f"twin rows ({ties} ties, {dedupes} dedupes, {selfs} self drops)")


def small_world(d: int, metric: int):
    """n = 40 on one level of cap 16: ring links plus chords, every node reachable; rows 5 and 9 hold 3e38."""
    from tests.util import clustered

    n = 40
    x = clustered(n, d, 21 + d, n_centers=4, sigma=0.5)
    x[5] = 3e38
    x[9] = 3e38
    adj = np.full((n, 16), -1, np.int32)
    for v in range(n):
        adj[v, :6] = [(v + 1) % n, (v - 1) % n, (v + 7) % n, (v - 7) % n, (v + 13) % n, (v + 20) % n]
    return x, [(None, adj)], 0


def case_overflow(ref, device, d, metric, f16):
    """n = 40, efSearch 64, kk = 39: one table row holds 3e38, so its L2 distances overflow, and its inner products with a second such row
    are not finite.  The non-finite entries reach S and come out empty, in both modes."""
    x, levels, entry = small_world(d, metric)
    out = []
    for replace in (False, True):
        L = Level(x, levels, entry, metric, f16, device)
        batch = np.arange(40, dtype=np.int32)
        r = run_insert(ref, L, batch, replace, 39, 8, 1.0, 64)
        sd, sl = r["S"]
        bad = (sl >= 0) & ~np.isfinite(sd)
        assert bad.any() and (sl >= 0).sum(1).max() == 39, (int(bad.sum()), (sl >= 0).sum(1).max())  # non-finite entries did reach S
        _contract_checks(r, L, batch, replace, 39, 8)  # (every candidate that is left has a finite distance)
        if not replace:
            assert (r["got"][0][bad] == -1).all() and (r["got"][0][(sl >= 0) & ~bad] >= 0).all()
        assert not np.isfinite(r["before"][1][(r["before"][0] >= 0)]).all()  # ... and stored slots hold some too
        out.append(_finish(r, f"overflow replace={int(replace)} ({int(bad.sum())} non-finite in S)"))
        L.close()
    return "; ".join(out)


def case_void_and_duplicates(ref, device, d, metric, f16):
    """Two void ids (-1 and n + 5) and one id listed twice, in both modes."""
    x, levels, entry, marks = layered_graph(d, metric)
    out = []
    for replace in (True, False):
        L = Level(x, levels, entry, metric, f16, device)
        batch = np.array([17, -1, 902, N + 5, 17, marks[0], 3], np.int32)
        r = run_insert(ref, L, batch, replace, 10, 4, 1.0, 40)
        _contract_checks(r, L, batch, replace, 10, 4)
        cand = r["got"][0]
        assert (cand[[1, 3]] == -1).all() and cand[0].tobytes() == cand[4].tobytes() and (cand[0] >= 0).any()
        out.append(_finish(r, f"void + duplicate replace={int(replace)}"))
        L.close()
    return "; ".join(out)


def case_alpha(ref, device, d, metric, f16):
    """alpha = 1.2: the relaxed pass keeps more than the strict rule alone."""
    x, levels, entry, marks = layered_graph(d, metric)
    kept = []
    batch = np.arange(100, 172, dtype=np.int32)  # (72 rows are enough for the relaxed pass to show)
    for alpha in (1.0, 1.2):
        L = Level(x, levels, entry, metric, f16, device)
        r = run_insert(ref, L, batch, True, 30, 8, alpha, 40)
        _contract_checks(r, L, batch, True, 30, 8)
        kept.append(int(r["got"][2].sum()))
        line = _finish(r, f"alpha={alpha}")
        L.close()
    assert kept[1] > kept[0], kept
    return line + f" (strict {kept[0]}, relaxed {kept[1]})"


def case_m_above_candidates(ref, device, d, metric, f16):
    """m = 20 > K = 5: the edge slots beyond the kept ones are all invalid; the rows still get their links."""
    x, levels, entry, _ = layered_graph(d, metric)
    lv, ids = emptied(levels, x, metric, 70, 9)
    L = Level(x, lv, entry, metric, f16, device)
    r = run_insert(ref, L, ids, False, 5, 20, 1.0, 40)
    _contract_checks(r, L, ids, False, 5, 20)
    assert r["got"][0].shape[1] == 5 and (r["got"][5][ids] > 0).all() and (r["got"][5][ids] <= 5 + 70).all()
    line = _finish(r, "m > candidates")
    r2 = run_insert(ref, L, ids[:9], False, 5, 20, 1.0, 40, outputs=False)  # the optional outputs left out, on the handle that has grown
    assert not r2["diff"] and r2["stats_equal"]
    L.close()
    return line


EDGE_CASES = {"insert_300": case_insert_300, "refine_257": case_refine_257, "refine_k512": case_refine_k512, "twin_rows": case_twin_rows, "overflow": case_overflow,
              "void_and_duplicates": case_void_and_duplicates, "alpha": case_alpha, "m_above_candidates": case_m_above_candidates}


def case_rejections(ref, device, d=64, metric=1, f16=False):
    """Every rejection the header lists: the code, and pre-filled d_adj / d_dist / d_deg and optional outputs byte for byte afterwards.
    Nothing is launched.  Then b == 0: LM_OK, nothing written."""
    import torch

    from leann_amd import _lib
    from leann_amd.index import Mi355xIndex

    lib = _lib.load()
    x, levels, entry, _ = layered_graph(d, metric)
    L = Level(x, levels, entry, metric, f16, device)
    n, cap, b, kk, m = L.n, 16, 5, 6, 4
    batch = L.tensor(np.array([1, 2, 3, 4, 5], np.int32))
    other = L.tensor(L.arrays()[0])  # the same contents at another address
    state = L.arrays()

    def outs(K):
        return (L.tensor(np.full((b, K), FILL_I32, np.int32)), L.tensor(np.full((b, K), FILL_F32, np.float32)), L.tensor(np.full((b, K), FILL_U8, np.uint8)))

    def ptr(t):
        return None if t is None else C.c_void_p(t.data_ptr())

    def call(h=None, bt=batch, nb=b, replace=1, kk_=kk, m_=m, alpha=1.0, prm=None, null_prm=False, adj="own", dist="own", deg="own", **pk):
        K = max(1, min(kk_ + (cap if replace == 1 else 0), 600))
        o = outs(K)
        p = L.idx.make_params(**dict(dict(ef=16, beam=2, recompute=False), **pk)) if prm is None else prm
        rc = lib.lm_graph_insert_batch(L.idx._h if h is None else h, ptr(bt), nb, replace, kk_, m_, alpha, None if null_prm else C.byref(p),
                                       ptr(L.adj if adj == "own" else adj), ptr(L.dist if dist == "own" else dist), ptr(L.deg if deg == "own" else deg), *[ptr(t) for t in o])
        now = L.arrays()
        same = all(u.tobytes() == v.tobytes() for u, v in zip(now, state)) and bool((o[0].cpu().numpy() == FILL_I32).all()) and \
            bool((o[1].cpu().numpy() == FILL_F32).all()) and bool((o[2].cpu().numpy() == FILL_U8).all())
        return rc, same

    EINVAL, ESTATE = _lib.LM_EINVAL, _lib.LM_ESTATE
    bad = [(EINVAL, dict(h=C.c_void_p(None))), (EINVAL, dict(null_prm=True)), (EINVAL, dict(adj=None)), (EINVAL, dict(dist=None)), (EINVAL, dict(deg=None)),
           (EINVAL, dict(bt=None)), (EINVAL, dict(nb=-1)), (EINVAL, dict(nb=(1 << 30) // m + 1)), (EINVAL, dict(nb=1 << 40)), (EINVAL, dict(replace=2)),
           (EINVAL, dict(replace=-1)), (EINVAL, dict(kk_=0)), (EINVAL, dict(kk_=-3)), (EINVAL, dict(m_=0)), (EINVAL, dict(kk_=_lib.SELECT_MAX_K + 1, replace=0)),
           (EINVAL, dict(kk_=_lib.SELECT_MAX_K - cap + 1)), (EINVAL, dict(alpha=0.99)), (EINVAL, dict(alpha=float("nan"))), (EINVAL, dict(alpha=float("inf"))),
           (EINVAL, dict(adj=other)), (ESTATE, dict(recompute=True)), (ESTATE, dict(batch_size=4)), (EINVAL, dict(batch_size=-1)), (ESTATE, dict(prune_ratio=0.5)),
           (EINVAL, dict(ef=9600)), (EINVAL, dict(beam=65)), (EINVAL, dict(ef=0))]
    for code, over in bad:
        rc, same = call(**over)
        assert rc == code and same, (over, rc, same, lib.lm_last_error())
    L.idx.set_option("persistent_table", 0)
    assert call() == (ESTATE, True)
    L.idx.set_option("persistent_table", 1)
    # a handle that is not a view; a view without a table
    from tests.view_ref_util import compose_csr

    csr = Mi355xIndex.from_csr(compose_csr(levels, n, d, metric, entry))
    csr.attach_table(L.table[:, :d].astype(np.float32))
    assert call(h=csr._h) == (ESTATE, True)
    csr.close()
    bare = Level(x, levels, entry, metric, f16, device, attach=False)
    rc = lib.lm_graph_insert_batch(bare.idx._h, ptr(batch), b, 1, kk, m, 1.0, C.byref(bare.idx.make_params(ef=16, beam=2, recompute=False)), ptr(bare.adj), ptr(bare.dist),
                                   ptr(bare.deg), None, None, None)
    assert rc == ESTATE and all(u.tobytes() == v.tobytes() for u, v in zip(bare.arrays(), state))
    bare.close()
    # b == 0: fine with and without a batch pointer, nothing written
    assert call(nb=0) == (_lib.LM_OK, True) and call(nb=0, bt=None) == (_lib.LM_OK, True)
    L.close()
    return "rejections and b = 0: ok"


def csr_equal(a, b) -> bool:
    return (a.ntotal == b.ntotal and a.entry_point == b.entry_point and a.max_level == b.max_level and a.levels.tobytes() == b.levels.tobytes()
            and a.level_ptr.tobytes() == b.level_ptr.tobytes() and a.node_offsets.tobytes() == b.node_offsets.tobytes() and a.neighbors.tobytes() == b.neighbors.tobytes())


def build_both(xt, metric: str, seed_nodes: int):
    """build_graph_gpu (M = 8, ef_construction = 40; selector, linker, search = kernel, kernel, view) with inserter="torch" and "kernel".
    -> (graph torch, graph kernel, counts): counts = calls of _LevelView.search / _LevelView.insert on each path."""
    from leann_amd import gpu_graph_build as gb

    counts = {"torch": [0, 0], "kernel": [0, 0]}
    real_search, real_insert = gb._LevelView.search, gb._LevelView.insert
    graphs = {}
    for which in ("torch", "kernel"):
        def search(self, *a, _w=which, **k):
            counts[_w][0] += 1
            return real_search(self, *a, **k)

        def insert(self, *a, _w=which, **k):
            counts[_w][1] += 1
            return real_insert(self, *a, **k)

        gb._LevelView.search, gb._LevelView.insert = search, insert
        try:
            graphs[which] = gb.build_graph_gpu(xt, metric, M=8, ef_construction=40, seed_nodes=seed_nodes, selector="kernel", linker="kernel", search="view", inserter=which)
        finally:
            gb._LevelView.search, gb._LevelView.insert = real_search, real_insert
    return graphs["torch"], graphs["kernel"], counts
