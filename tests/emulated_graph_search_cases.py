"""Edge cases of the graph search (lm_index_search: k_expand, k_update, k_search_table, k_uniq_count / k_uniq_emit and the shared blocks of
csrc/lm_beam_common.h) against oracle/lm_oracle.c: labels, distance BITS, ndis / nexpand / nrounds and, in provider mode, the request list
of every round -- no tolerance anywhere.  The shapes, inputs and the premises asserted from them live here;
tests/test_gpu_graph_search_edges.py runs them on the MI355X, tests/test_graph_search_edges.py against the host build of the library
(tests/hip_emul/build_emul_lib.py):
    python -m tests.emulated_graph_search_cases <path/to/libleann_mi355x_emul.so> [case ...]
The graphs are small hand-built CSR graphs from seeded generators, so that the shapes are there by construction and not by luck of a build.

A "world" is one way through the launchers: the persistent kernel or the lock-step rounds, each with a workgroup or a wave per query, over
the stored table; and in provider mode the rank addressing (workgroup / wave), the rank addressing with `identity` (option
single_query_direct, one query at a time) and the memo slot.  The GPU runs every scenario in every world it can take; the host build runs
each scenario in a subset, the whole set walked across the scenarios of a case (case A excepted: there a form IS a world, all run).

The host build differs in size only: case A 150 points instead of 600, case D 300 nodes instead of 1200; case E (N = 262181) runs its
searches there too, without the hub cache part's device tensors (the host build takes host pointers: the backend hands them over)."""
import ctypes as C
import re
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
SEARCH_SRC = ROOT / "leann_amd" / "csrc" / "lm_search.hip"
IP, L2 = 0, 1
METRIC_NAME = {IP: "mips", L2: "l2"}
PERSIST_LDS, LOCKSTEP_LDS = 150 * 1024, 64 * 1024   # search_lds_checks (lm_search.hip)
UNIQ_TILE_NODES = 4096 * 32                          # UNIQ_TILE words of the request bitmap (lm_device_types.h)
TABLE_WORLDS = ("persist_wg", "persist_wave", "lock_wg", "lock_wave")
PROVIDER_WORLDS = ("rank_wg", "rank_wave", "identity", "memo")
WORLDS = TABLE_WORLDS + PROVIDER_WORLDS
CASES = {}
_CACHE = {}


def _load(lib_path: str):
    from leann_amd import _lib

    _lib.LIB_PATH = Path(lib_path)
    _lib._lib = None
    return _lib.load()


# ---- the two libraries -----------------------------------------------------------------------------------------------------------
class HostBackend:
    """The host build of the library: 'device' pointers are host pointers."""

    emulated = True

    def prepare(self, idx):
        pass

    def provider(self, x, dp):
        xp = np.zeros((x.shape[0], dp), np.float32)
        xp[:, : x.shape[1]] = x
        calls, keep = [], {}

        def fn(d_ids, n, stream):
            ids = np.ctypeslib.as_array(C.cast(d_ids, C.POINTER(C.c_int32)), shape=(n,)).copy()
            calls.append(ids)
            keep["e"] = np.ascontiguousarray(xp[ids])
            return keep["e"].ctypes.data

        return fn, calls

    def set_hub_cache(self, idx, ids, rows):
        from leann_amd import _lib

        ids, rows = np.ascontiguousarray(ids, np.int32), np.ascontiguousarray(rows, np.float32)
        _lib.check(idx._lib.lm_index_set_hub_cache(idx._h, ids.ctypes.data_as(C.c_void_p), len(ids), rows.ctypes.data_as(C.c_void_p)), "lm_index_set_hub_cache")


class GpuBackend:
    emulated = False

    def prepare(self, idx):
        import torch

        idx.set_stream(torch.cuda.current_stream().cuda_stream)

    def provider(self, x, dp):
        import torch

        from leann_amd.devmem import as_tensor

        xdev = torch.zeros((x.shape[0], dp), device="cuda")
        xdev[:, : x.shape[1]] = torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
        calls, keep = [], {}

        def fn(d_ids, n, stream):
            ids = as_tensor(d_ids, (n,), "int32")
            calls.append(ids.cpu().numpy().copy())
            keep["e"] = xdev.index_select(0, ids.long()).contiguous()
            return keep["e"].data_ptr()

        return fn, calls

    def set_hub_cache(self, idx, ids, rows):
        import torch

        idx.set_hub_cache(np.ascontiguousarray(ids, np.int32), torch.from_numpy(np.ascontiguousarray(rows, np.float32)).cuda().contiguous())


# ---- graphs ------------------------------------------------------------------------------------------------------------------------
def make_csr(levels_adj, d, metric, entry_point):
    """A compact CSR (convert_to_csr.py layout) from per-level neighbour lists kept exactly as given (duplicates, self loops, empty
    lists): levels_adj[0] is a list of n arrays, levels_adj[l > 0] a dict node -> array; a node has the levels up to its highest dict."""
    from leann_amd.csr_format import HnswCsr

    n = len(levels_adj[0])
    levels = np.ones(n, np.int32)
    for l in range(1, len(levels_adj)):
        for v in levels_adj[l]:
            levels[v] = max(levels[v], l + 1)
    empty = np.zeros(0, np.int32)
    lists, level_ptr, pos = [], [], 0
    for i in range(n):
        for l in range(int(levels[i])):
            a = np.asarray(levels_adj[0][i] if l == 0 else levels_adj[l].get(i, empty), np.int32).reshape(-1)
            level_ptr.append(pos)
            lists.append(a)
            pos += a.size
        level_ptr.append(pos)
    nb = np.concatenate(lists + [empty]).astype(np.int32)
    assert nb.size == 0 or (0 <= nb.min() and nb.max() < n)  # the kernels dereference every id
    node_offsets = np.concatenate([[0], np.cumsum(levels.astype(np.int64) + 1)]).astype(np.uint64)
    max_level = len(levels_adj) - 1
    assert levels[entry_point] == max_level + 1
    return HnswCsr(d=d, ntotal=n, metric_type=metric, levels=levels, level_ptr=np.asarray(level_ptr, np.uint64), node_offsets=node_offsets,
                   neighbors=nb, entry_point=int(entry_point), max_level=max_level)


def flat_csr_arrays(deg, nb, d, metric, entry_point):
    """make_csr for ONE level from the degree array and the concatenated lists (vectorised: case E has 262181 nodes)."""
    from leann_amd.csr_format import HnswCsr

    n = deg.shape[0]
    cs = np.cumsum(deg.astype(np.int64))
    level_ptr = np.zeros(2 * n, np.uint64)
    level_ptr[0::2] = cs - deg
    level_ptr[1::2] = cs
    assert nb.shape[0] == cs[-1] and 0 <= nb.min() and nb.max() < n
    return HnswCsr(d=d, ntotal=n, metric_type=metric, levels=np.ones(n, np.int32), level_ptr=level_ptr, node_offsets=np.arange(n + 1, dtype=np.uint64) * 2,
                   neighbors=np.ascontiguousarray(nb, np.int32), entry_point=int(entry_point), max_level=0)


def nbr_list(g, node, level):
    p = int(g.node_offsets[node]) + level
    return g.neighbors[int(g.level_ptr[p]) : int(g.level_ptr[p + 1])]


def layered_graph(n, d, metric, seed, deg_lo=3, deg_hi=12):
    """Three levels: level 0 a ring plus deg_lo .. deg_hi - 1 distinct random links per node, level 1 every 8th node, level 2 every 64th;
    entered at node 0."""
    rng = np.random.default_rng(seed)
    adj0 = []
    for i in range(n):
        c = rng.choice(n - 1, int(rng.integers(deg_lo, deg_hi)) - 1, replace=False)
        adj0.append(np.concatenate([[(i + 1) % n], np.where(c >= i, c + 1, c)]).astype(np.int32))
    ups = []
    for step, fan in ((8, 6), (64, 2)):
        nodes = np.arange(0, n, step)
        lv = {}
        for j, v in enumerate(nodes):
            others = np.delete(nodes, j)
            lv[int(v)] = np.unique(np.concatenate([[nodes[(j + 1) % len(nodes)]], rng.choice(others, min(fan, len(others)), replace=False)])).astype(np.int32)
        ups.append(lv)
    return make_csr([adj0] + ups, d, metric, 0)


# ---- comparison ------------------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_result(tag, got, st, exp):
    """(distances, labels) and the stats of a call against the oracle's (ids, distances, stats): everything equal."""
    (gd, gi), (oi, od, ost) = got, exp
    nl, nd = int((gi != oi).sum()), int((_bits(gd) != _bits(od)).sum())
    assert nl == 0 and nd == 0, (tag, f"{nl} labels and {nd} distance words of {gi.size} differ", np.argwhere(gi != oi)[:4].tolist())
    have = tuple(int(st[f]) for f in ("ndis", "nexpand", "nrounds"))
    assert have == (ost["ndis"], ost["nexpand"], ost["nrounds"]), (tag, "ndis / nexpand / nrounds", have, ost)


def check_requests(tag, seen, want, sort_seen=False):
    assert len(seen) == len(want), (tag, "provider calls", len(seen), len(want))
    for r, (a, b) in enumerate(zip(seen, want)):
        if sort_seen:
            assert np.unique(a).shape[0] == a.shape[0], (tag, "a node twice in one request list", r)
            a = np.sort(a)
        assert np.array_equal(a, b), (tag, f"round {r}: the provider was not asked for the oracle's ids")


def raw_search(idx, q, k, prm):
    """lm_index_search into PRE-FILLED outputs -> (rc, distances, labels, lm_last_error): what a refused call must leave untouched."""
    from leann_amd import _lib

    q = np.ascontiguousarray(q, np.float32)
    dist, labels = np.full((q.shape[0], k), 123.25, np.float32), np.full((q.shape[0], k), -77, np.int64)
    rc = idx._lib.lm_index_search(idx._h, q.shape[0], q.ctypes.data_as(C.c_void_p), k, dist.ctypes.data_as(C.c_void_p), labels.ctypes.data_as(C.c_void_p), C.byref(prm))
    return rc, dist, labels, _lib.last_error()


def assert_refused(tag, idx, q, k, prm):
    from leann_amd import _lib

    rc, dist, labels, err = raw_search(idx, q, k, prm)
    assert rc == _lib.LM_EINVAL and "LDS" in err, (tag, rc, err)
    assert np.all(dist == np.float32(123.25)) and np.all(labels == -77), (tag, "a refused call wrote to its outputs")


class Scenario:
    """One (graph, table, queries, k, efSearch, beam, stop rule, batch_size) with the oracle's answers (computed once, kept unchanged)."""

    def __init__(self, tag, g, x, q, k, ef, beam=1, check_rel=True, batch_size=0):
        from tests.util import oracle_graph

        self.tag, self.g, self.x, self.q, self.k, self.ef, self.beam, self.check_rel, self.batch_size = tag, g, x, np.ascontiguousarray(q, np.float32), k, ef, beam, check_rel, batch_size
        self.og = oracle_graph(g, x.shape[1])
        self._exp = {}

    def _kw(self):
        return dict(ef=self.ef, beam=self.beam, check_relative_distance=self.check_rel, batch_size=self.batch_size)

    def table(self, f16=False):
        from oracle import oracle as orc

        if ("table", f16) not in self._exp:
            tab = self.x.astype(np.float16).astype(np.float32) if f16 else self.x
            self._exp[("table", f16)] = orc.search(self.og, self.q, self.k, table=tab, **self._kw())
        return self._exp[("table", f16)]

    def provider(self, memo, rows=None):
        """-> (ids, dist, stats, request lists of the rounds); rows: the queries of the call (None = all)."""
        from oracle import oracle as orc

        key = ("provider", memo, None if rows is None else tuple(rows))
        if key not in self._exp:
            want = []
            q = self.q if rows is None else self.q[list(rows)]
            r = orc.search(self.og, q, self.k, memo=memo, provider=lambda idv: (want.append(idv.copy()), self.x[idv])[1], **self._kw())
            self._exp[key] = r + (want,)
        return self._exp[key]

    def params(self, idx, recompute, memo=False):
        return idx.make_params(ef=self.ef, beam=self.beam, check_relative_distance=self.check_rel, recompute=recompute, recompute_memo=memo, batch_size=self.batch_size)

    def worlds(self):
        """The worlds this scenario can take: the persistent launch serves beam <= 64 without dynamic batching (else the call would run the
        lock-step rounds under another name); the memo is used by a call of more than one query."""
        out = [w for w in WORLDS if not (w.startswith("persist") and (self.beam > 64 or self.batch_size > 0))]
        return [w for w in out if not (w == "memo" and self.q.shape[0] < 2)]

    def run(self, be, worlds=None, f16s=(False,), idx=None):
        from leann_amd.index import Mi355xIndex

        own = idx is None
        if own:
            idx = Mi355xIndex.from_csr(self.g)
            be.prepare(idx)
        try:
            for w in (self.worlds() if worlds is None else worlds):
                assert w in self.worlds(), (self.tag, w)
                for f16 in (f16s if w in TABLE_WORLDS else (False,)):
                    self._run_world(be, idx, w, f16)
        finally:
            if own:
                idx.close()

    def _run_world(self, be, idx, w, f16):
        tag = (self.tag, w, "f16" if f16 else "f32")
        idx.set_option("single_query_direct", 0)
        if w in TABLE_WORLDS:
            idx.attach_table(self.x.astype(np.float16) if f16 else self.x)
            idx.set_option("persistent_table", 1 if w.startswith("persist") else 0)
            idx.set_option("update_variant", {"persist_wg": 0, "persist_wave": 0, "lock_wg": 4, "lock_wave": 3}[w])
            idx.set_option("persistent_wave", 1 if w == "persist_wave" else 0)
            check_result(tag, idx.search(self.q, self.k, self.params(idx, False)), idx.stats(), self.table(f16))
            return
        fn, calls = be.provider(self.x, int(idx.info.d_padded))
        idx.set_provider(fn)
        idx.set_option("update_variant", 3 if w == "rank_wave" else 4)
        if w == "identity":  # one query at a time: the new-list is the request list, in discovery order
            idx.set_option("single_query_direct", 1)
            for i in range(self.q.shape[0]):
                calls.clear()
                exp = self.provider(False, (i,))
                check_result(tag + (i,), idx.search(self.q[i : i + 1], self.k, self.params(idx, True, False)), idx.stats(), exp[:3])
                check_requests(tag + (i,), calls, exp[3], sort_seen=True)
                assert int(idx.stats()["nunique"]) == exp[2]["nunique"], tag
            idx.set_option("single_query_direct", 0)
        else:
            memo = w == "memo"
            exp = self.provider(memo)
            check_result(tag, idx.search(self.q, self.k, self.params(idx, True, memo)), idx.stats(), exp[:3])
            check_requests(tag, calls, exp[3])
            assert int(idx.stats()["nunique"]) == exp[2]["nunique"], (tag, int(idx.stats()["nunique"]), exp[2])
            if memo:
                allids = np.concatenate(calls)
                assert np.unique(allids).shape[0] == allids.shape[0], (tag, "a node reached the provider twice in one call")
        idx.set_provider(None)


# ---- a validated restatement of one query's walk: what the premises read ---------------------------------------------------------------
def query_distances(x, q1, metric):
    """Internal distances (smaller is better) of every row to ONE query as the key orders them (NaN as +inf, -0 as +0): the oracle's own
    exhaustive ranking, scattered back by id."""
    from oracle import oracle as orc

    ids, dd = orc.bruteforce_topk(x, q1[None], x.shape[0], metric)
    out = np.empty(x.shape[0], np.float64)
    out[ids[0]] = dd[0] if metric == L2 else -dd[0].astype(np.float64)
    return out + 0.0


def walk(g, dint, ef_s, k, W, check_rel):
    """The rounds of one query under the contract of oracle/lm_oracle.c's header, with what the oracle does not report: the pops of every
    round, their lists, the gathered slots, the pool size in front of the merge.  validated_walk holds it to the oracle."""
    ef = max(ef_s, k)
    key = lambda v: (float(dint[v]), int(v))  # noqa: E731
    rounds = [dict(phase="seed", pops=[], lists=[], new=[g.entry_point], slots=1, npool0=0)]
    cur, level = g.entry_point, g.max_level
    while level > 0:
        lst = [int(v) for v in nbr_list(g, cur, level)]
        rounds.append(dict(phase="upper", pops=[cur], lists=[lst], new=lst, slots=len(lst), npool0=0))
        best = min(lst, key=key) if lst else None
        if best is not None and key(best) < key(cur):
            cur = best
        else:
            level -= 1
    visited, pool, nsteps = {cur}, [[key(cur), False]], 0
    selects = []

    def select():
        nonlocal nsteps
        pops, start = [], nsteps
        for i, e in enumerate(pool):
            if len(pops) >= W:
                break
            if e[1]:
                continue
            if (check_rel and i >= ef_s) or (not check_rel and nsteps > ef_s):
                break
            e[1] = True
            pops.append(e[0][1])
            nsteps += 1
        selects.append(dict(allowed=W if check_rel else min(W, max(0, ef_s + 1 - start)), found=len(pops),
                            unexpanded_left=sum(1 for e in pool if not e[1]), unexpanded_beyond_efs=sum(1 for e in pool[ef_s:] if not e[1])))
        return pops

    pops = select()
    seed0 = cur
    while pops:
        lists, new = [[int(v) for v in nbr_list(g, p, 0)] for p in pops], []
        for lst in lists:
            for v in lst:
                if v not in visited:
                    visited.add(v)
                    new.append(v)
        rounds.append(dict(phase="beam", pops=pops, lists=lists, new=new, slots=sum(len(l) for l in lists), npool0=len(pool)))
        pool = sorted(pool + [[key(v), False] for v in new], key=lambda e: e[0])[:ef]
        pops = select()
    return dict(rounds=rounds, selects=selects, labels=[e[0][1] for e in pool[:k]], seed0=seed0, visited=visited)


def validated_walk(sc, i):
    """walk() of query i of a scenario, asserted equal to the oracle's one-query provider run: request list of every round, labels, ndis,
    nexpand, nrounds."""
    key = ("walk", i)
    if key not in sc._exp:
        oi, _, ost, want = sc.provider(False, (i,))
        w = walk(sc.g, query_distances(sc.x, sc.q[i], sc.g.metric_type), sc.ef, sc.k, sc.beam, sc.check_rel)
        mine = [np.unique(np.asarray(r["new"], np.int32)) for r in w["rounds"] if len(r["new"])]
        assert len(mine) == len(want) and all(np.array_equal(a, b) for a, b in zip(mine, want)), (sc.tag, i, "the restated walk left the oracle's trace")
        lab = w["labels"] + [-1] * (sc.k - len(w["labels"]))
        assert lab == oi[0].tolist(), (sc.tag, i)
        assert (sum(len(r["new"]) for r in w["rounds"]), sum(len(r["pops"]) for r in w["rounds"] if r["phase"] == "beam"), len(w["rounds"])) == \
            (ost["ndis"], ost["nexpand"], ost["nrounds"]), (sc.tag, i, ost)
        sc._exp[key] = w
    return sc._exp[key]


def next_pow2(v):
    p = 1
    while p < v:
        p <<= 1
    return p


# ---- case A: every form the launchers can reach -------------------------------------------------------------------------------------------
WIDTHS = (1, 2, 3, 4, 5, 6, 8, 12, 16)  # NCH = padded width / 64: the CASE labels of launch_update_nch and launch_persist_nch


def forms():
    """The launchers' selection rule as a list.  Table mode: (NCH, L2, F16) x {persistent, lock-step} x {256, 64 threads}; provider mode
    (fp32 rows): rank addressing at 256 and 64 threads, the same with `identity`, the memo slot (256 threads only: launch_update_nch).
    Each form: (world, nch, l2, f16, kernel, template values) -- template values as the source spells the instantiation."""
    out = []
    for nch in WIDTHS:
        for l2 in (False, True):
            for f16 in (False, True):
                out.append(("persist_wg", nch, l2, f16, "k_search_table", (256,)))
                out.append(("persist_wave", nch, l2, f16, "k_search_table", (64,)))
                out.append(("lock_wg", nch, l2, f16, "k_update", (0, 256)))
                out.append(("lock_wave", nch, l2, f16, "k_update", (0, 64)))
            out.append(("rank_wg", nch, l2, False, "k_update", (1, 256)))
            out.append(("rank_wave", nch, l2, False, "k_update", (1, 64)))
            out.append(("identity", nch, l2, False, "k_update", (1, 256)))
            out.append(("memo", nch, l2, False, "k_update", (2, 256)))
    return out


def launcher_instantiations():
    """Read from csrc/lm_search.hip: the CASE labels of the two launchers, the (MODE, NT) / NT values their macros instantiate and the
    (L2, F16) pairs their callers pass."""
    src = SEARCH_SRC.read_text()
    upd = src[src.index("static int launch_update_nch") : src.index("static int launch_update(")]
    per = src[src.index("static int launch_persist_nch") : src.index("#define VIEW_LDS_TEXT")]
    caller = src[src.index("static int launch_update(") : src.index("struct FilterPass")]
    return dict(update_labels={int(v) for v in re.findall(r"\bCASE\((\d+)\)", upd)}, persist_labels={int(v) for v in re.findall(r"\bCASEP\((\d+)\)", per)},
                update_forms={(int(m), int(nt)) for m, nt in re.findall(r"k_update<n, L2, F16, (\d), (\d+)>", upd)},
                persist_forms={(int(nt),) for nt in re.findall(r"k_search_table<n, L2, F16, (\d+), GA>", per)},
                update_types={(a == "true", b == "true") for a, b in re.findall(r"launch_update_nch<(true|false), (true|false)>", caller)},
                persist_types={(a == "true", b == "true") for a, b in re.findall(r"launch_persist_nch<(true|false), (true|false)>", src)})


def assert_forms_cover_every_instantiation(form_list=None):
    """Every CASE label and every template parameter value of the two launchers has a form (and the list names nothing the source lacks)."""
    fl = forms() if form_list is None else form_list
    src = launcher_instantiations()
    both = {(False, False), (False, True), (True, False), (True, True)}
    assert src["update_types"] == both and src["persist_types"] == both, src
    assert src["update_forms"] == {(0, 256), (0, 64), (1, 256), (1, 64), (2, 256)} and src["persist_forms"] == {(256,), (64,)}, src
    for kernel, labels, tvals in (("k_update", src["update_labels"], src["update_forms"]), ("k_search_table", src["persist_labels"], src["persist_forms"])):
        have = {(f[1], f[2], f[3], f[5]) for f in fl if f[4] == kernel}
        # fp16 rows exist in table mode only (search_pass passes f16 = false with a provider): MODE 1 / 2 with F16 are compiled, never launched
        need = {(n, l2, f16, t) for n in labels for l2 in (False, True) for f16 in (False, True) for t in tvals if not (f16 and kernel == "k_update" and t[0] != 0)}
        assert need <= have, (kernel, "instantiations without a form", sorted(need - have)[:6])
        assert have <= need, (kernel, "forms without an instantiation", sorted(have - need)[:6])
    assert any(f[0] == "identity" for f in fl)


def forms_world(nch, metric, emulated):
    """About 600 (host build: 150) points, not normalised, d = 64 nch - 3 so that the padded tail is live, 9 queries."""
    key = ("A", nch, metric, emulated)
    if key not in _CACHE:
        n, d = (150 if emulated else 600), 64 * nch - 3
        rng = np.random.default_rng(1000 + 2 * nch + metric)
        x = (1.5 * rng.standard_normal((n, d))).astype(np.float32)
        q = (x[rng.integers(0, n, 9)] + 0.4 * rng.standard_normal((9, d))).astype(np.float32)
        _CACHE[key] = Scenario(("forms", 64 * nch, METRIC_NAME[metric]), layered_graph(n, d, metric, 2000 + nch), x, q, 10, 32, beam=2)
    return _CACHE[key]


def assert_every_chunk_matters(sc):
    """Zeroing any one 64-wide chunk of the rows changes the oracle's labels for some query: a form that skipped or repeated a chunk, or
    strode its rows wrongly, cannot return the right neighbours."""
    from oracle import oracle as orc

    base = sc.table()[0]
    d = sc.x.shape[1]
    for c in range((d + 63) // 64):
        y = sc.x.copy()
        y[:, 64 * c : 64 * (c + 1)] = 0
        assert not np.array_equal(orc.search(sc.og, sc.q, sc.k, table=y, **sc._kw())[0], base), (sc.tag, "chunk", c)


def case_every_form(be, widths=None):
    """Case A."""
    done = []
    for nch in WIDTHS:
        if widths is not None and nch not in widths:
            continue
        for metric in (IP, L2):
            sc = forms_world(nch, metric, be.emulated)
            assert sc.x.shape[1] == 64 * nch - 3 and sc.q.shape[0] == 9
            assert_every_chunk_matters(sc)
            sc.run(be, f16s=(False, True))
            done += [f for f in forms() if f[1] == nch and f[2] == (metric == L2)]
        print(f"forms width {64 * nch}: ok", flush=True)
    return done


CASES["every_form"] = case_every_form


# ---- case B: both merge branches, at both widths --------------------------------------------------------------------------------------------
def counting_pays(nt, npool0, n):
    """rank_merge_unsorted_pays<NT> (lm_beam_common.h) at the library's limit."""
    return n * ((n + npool0 + nt - 1) // nt) <= 256


MERGE_EF = 96


def merge_hops():
    """New nodes per hop of the hub chain, chosen from the rule itself: a first hop of more than 256; with the pool full (npool0 = ef = 96)
    the largest n that still counts and the next one, for 64 and for 256 threads; exact powers of two and 2^m + 1 on the sorting side."""
    edge = {nt: max(n for n in range(1, 600) if counting_pays(nt, MERGE_EF, n)) for nt in (64, 256)}
    return [301, 256, 257, edge[256], edge[256] + 1, edge[64], edge[64] + 1, 128, 129, 3, 17, 64, 65, 5], edge


def merge_world():
    """A chain of hubs: hub i lists n_i - 1 leaves of its own and hub i + 1.  Every hub is nearer to the query than every leaf, so a
    beam-1 search expands hub after hub and round i evaluates exactly n_i new nodes (the last hub has only leaves); leaves list nothing."""
    if "B" not in _CACHE:
        hops, _ = merge_hops()
        rng = np.random.default_rng(77)
        d = 61
        q = rng.standard_normal(d).astype(np.float32)
        nh = len(hops)
        adj, rows = [None] * nh, []
        for i in range(nh):
            u = rng.standard_normal(d)
            rows.append(q + (0.5 + 0.1 * (nh - i)) * u / np.linalg.norm(u))
        nxt = nh
        for i, n_i in enumerate(hops):
            leaves = n_i - (1 if i + 1 < nh else 0)
            adj[i] = np.concatenate([np.arange(nxt, nxt + leaves), [i + 1] if i + 1 < nh else []]).astype(np.int32)
            nxt += leaves
        for _ in range(nxt - nh):
            u = rng.standard_normal(d)
            rows.append(q + rng.uniform(5.0, 10.0) * u / np.linalg.norm(u))
            adj.append(np.zeros(0, np.int32))
        x = np.asarray(rows, np.float32)
        g = make_csr([adj], d, L2, 0)
        _CACHE["B"] = (Scenario(("merge", 1), g, x, q[None], 10, MERGE_EF), Scenario(("merge", 2), g, x, np.stack([q, q]), 10, MERGE_EF))
    return _CACHE["B"]


def assert_merge_premises():
    """From the oracle's one-query provider trace (without a memo a round's request list IS the query's new-list): the (n, npool0) of every
    level-0 round fall on both sides of the rule for 64 and for 256 threads -- k_update and k_search_table decide by the same numbers --,
    and hold the shapes named above."""
    sc = merge_world()[0]
    hops, edge = merge_hops()
    want = sc.provider(False)[3]
    assert len(want[0]) == 1  # the seed (a single-level graph: every later round is a level-0 round)
    ns = [len(r) for r in want[1:]]
    assert ns == hops, (ns, hops)  # (rounds without a new node ask for nothing and merge nothing)
    npool0 = [min(MERGE_EF, 1 + sum(ns[:i])) for i in range(len(ns))]
    assert validated_walk(sc, 0)["rounds"][1]["npool0"] == 1 and [r["npool0"] for r in validated_walk(sc, 0)["rounds"][1 : 1 + len(ns)]] == npool0
    for nt in (64, 256):
        side = [counting_pays(nt, p, n) for n, p in zip(ns, npool0)]
        assert any(side) and not all(side), (nt, side)
        full = {n: counting_pays(nt, p, n) for n, p in zip(ns, npool0) if p == MERGE_EF}
        assert full[edge[nt]] and not full[edge[nt] + 1], (nt, edge)                                    # just under, just over, pool full
        assert any(not s and n & (n - 1) == 0 for n, s in full.items())                                 # a sort without padding
        assert any(not s and (n - 1) & (n - 2) == 0 and n > 2 for n, s in full.items())                 # a sort of 2^m + 1 keys
        assert any(s and (n - 1) & (n - 2) == 0 and n > 2 for n, s in full.items())                     # ... and counting of 2^m + 1
    assert ns[0] > 256 and next_pow2(ns[0]) == 512 and npool0[0] == 1 and not counting_pays(256, 1, ns[0])  # the first hop sorts at any width
    return ns, npool0


def case_merge_branches(be):
    """Case B."""
    assert_merge_premises()
    one, two = merge_world()
    one.run(be)
    two.run(be, worlds=("memo", "rank_wg", "persist_wg", "lock_wave") if be.emulated else None)
    print("merge branches at 64 and 256 threads: ok", flush=True)


CASES["merge_branches"] = case_merge_branches


# ---- case C: expansion edges -----------------------------------------------------------------------------------------------------------
EP, LONG64, LONG256, TWINS = 650, 20, 21, (40, 43)  # (the entry point's id above its neighbours': a tie on distance moves the descent)
SPECIAL_ROWS = (30, 31, 32, 33)  # a NaN, a +inf, a -inf coordinate; a row of -0


def edge_graph(metric, wide):
    """700 nodes, two levels.  Level 0: lists of 0 .. 8 ids drawn WITH replacement (duplicates, self loops, many empty lists); the entry
    point's list is empty; nodes 40 and 43 share an id, 40 lists it twice and itself.  wide: node 20 lists 70 distinct ids, node 21 lists 300
    ids with repeats and itself, and both are listed often; else no list is longer than 31 (beam 130 x 31 slots is what the lock-step LDS
    holds).  Level 1: the entry point lists 300 nodes, each of which lists three others.  The special rows are listed by every fifth node."""
    key = ("C", metric, wide)
    if key not in _CACHE:
        rng = np.random.default_rng(4100 + 10 * metric + wide)
        n, d = 700, 61
        adj = [rng.integers(0, n, int(rng.integers(0, 9))).astype(np.int32) for _ in range(n)]
        adj[40] = np.array([41, 41, 40, 42], np.int32)
        adj[43] = np.array([41, 42, 44], np.int32)
        for i in range(0, n, 5):
            adj[i] = np.append(adj[i], SPECIAL_ROWS[(i // 5) % 4]).astype(np.int32)
        for i in range(0, n, 9):
            adj[i] = np.append(adj[i], [40, 43]).astype(np.int32)
        if wide:
            adj[LONG64] = rng.choice(n, 70, replace=False).astype(np.int32)
            adj[LONG256] = np.append(rng.integers(0, n, 299), LONG256).astype(np.int32)
            for i in range(0, n, 7):
                adj[i] = np.append(adj[i], [LONG64, LONG256]).astype(np.int32)
        else:
            adj[LONG64] = rng.integers(0, n, 31).astype(np.int32)
        adj[EP] = np.zeros(0, np.int32)
        top = np.arange(100, 400)
        up = {int(v): rng.choice(top[top != v], 3, replace=False).astype(np.int32) for v in top}
        up[EP] = top.astype(np.int32)
        x = rng.standard_normal((n, d)).astype(np.float32)
        x[30, 3], x[31, 7], x[32, 9] = np.nan, np.inf, -np.inf
        x[33] = -0.0
        q = (x[[200, 450]] + 0.3 * rng.standard_normal((2, d))).astype(np.float32)
        q = np.concatenate([q, np.zeros((1, d), np.float32), x[EP : EP + 1]])
        _CACHE[key] = (make_csr([adj, up], d, metric, EP), x, np.ascontiguousarray(q, np.float32))
    return _CACHE[key]


# (name, wide graph, k, efSearch, beam, check_relative_distance)
EDGE_SHAPES = [
    ("beam64", False, 10, 128, 64, True), ("beam65", False, 10, 140, 65, True), ("beam130", False, 10, 200, 130, True),
    ("k>ef", False, 20, 8, 2, True), ("k==ef", False, 16, 16, 3, True), ("ef1", False, 1, 1, 1, True), ("nstep-cut", False, 5, 6, 4, False),
    ("wide-beam8", True, 10, 64, 8, True), ("wide-beam1", True, 10, 32, 1, True), ("wide-nstep", True, 10, 40, 5, False),
]


def edge_scenarios():
    if "C-sc" not in _CACHE:
        out = []
        for name, wide, k, ef, beam, cr in EDGE_SHAPES:
            for metric in (IP, L2):
                g, x, q = edge_graph(metric, wide)
                out.append(Scenario(("edges", name, METRIC_NAME[metric]), g, x, q, k, ef, beam, cr))
        _CACHE["C-sc"] = out
    return _CACHE["C-sc"]


def assert_edge_premises():
    """Every shape the issue names occurs in some round of some query, read from the walks (each held to the oracle's trace)."""
    from oracle import oracle as orc

    seen = set()
    for sc in edge_scenarios():
        g, name = sc.g, sc.tag[1]
        assert len(nbr_list(g, EP, 0)) == 0 and len(nbr_list(g, EP, 1)) > 256 and int(g.entry_point) == EP
        if not np.isnan(sc.x[30, 3]) or sc.x[31, 7] != np.inf or sc.x[32, 9] != -np.inf or not np.all(np.signbit(sc.x[33])) or np.any(sc.q[2] != 0):
            raise AssertionError("special rows / zero query missing")
        for i in range(sc.q.shape[0]):
            w = validated_walk(sc, i)
            beams = [r for r in w["rounds"] if r["phase"] == "beam"]
            evaluated = {v for r in w["rounds"] for v in r["new"]}
            for s in SPECIAL_ROWS:
                if s in evaluated:
                    seen.add(("special", s, sc.g.metric_type, i == 2))
            if w["seed0"] == EP:
                seen.add("walk seeded at the entry point, whose list is empty")
                assert w["labels"] == [EP]
            for r in beams:
                np_, degs = len(r["pops"]), [len(l) for l in r["lists"]]
                if np_ == 64:
                    seen.add((name, "64 pops"))
                if np_ > 64:
                    seen.add((name, "more than 64 pops"))
                    if np_ % 64:
                        seen.add((name, "partial p0 pass"))
                if any(degs[j] == 0 and any(degs[:j]) and any(degs[j + 1 :]) for j in range(np_)):
                    seen.add("empty list between non-empty ones")
                if max(degs) > 64:
                    seen.add("list longer than 64")
                if max(degs) > 256:
                    seen.add("list longer than 256")
                if r["slots"] > 256 and len(r["new"]) < r["slots"]:
                    seen.add("more than 256 slots, fewer fresh")
                if any(len(set(l)) < len(l) for l in r["lists"]):
                    seen.add("id twice in one list")
                if any(p in l for p, l in zip(r["pops"], r["lists"])):
                    seen.add("self loop")
                if any(set(a) & set(b) for j, a in enumerate(r["lists"]) for b in r["lists"][j + 1 :]):
                    seen.add("same id in two lists of one round")
            last = w["selects"][-1]
            if sc.check_rel and sc.k > sc.ef and last["found"] == 0 and last["unexpanded_beyond_efs"] > 0:
                seen.add("count_below stops a pool with unexpanded entries")
            if not sc.check_rel and any(0 < s["allowed"] < sc.beam and s["found"] == s["allowed"] and s["unexpanded_left"] > 0 for s in w["selects"]):
                seen.add("nstep rule cuts a beam mid-round")
    need = {("beam64", "64 pops"), ("beam65", "more than 64 pops"), ("beam65", "partial p0 pass"), ("beam130", "more than 64 pops"), ("beam130", "partial p0 pass"),
            "empty list between non-empty ones", "list longer than 64", "list longer than 256", "more than 256 slots, fewer fresh", "id twice in one list",
            "self loop", "same id in two lists of one round", "walk seeded at the entry point, whose list is empty",
            "count_below stops a pool with unexpanded entries", "nstep rule cuts a beam mid-round"}
    assert need <= seen, sorted(map(str, need - seen))
    for s in SPECIAL_ROWS:  # every special row is evaluated under both metrics, and by the zero query under inner product
        assert ("special", s, IP, True) in seen and any(("special", s, L2, z) in seen for z in (False, True)), (s, sorted(map(str, seen)))
    # the raw distances really are the special values the key has to order: NaN (0 x inf, NaN coordinate), -0 (inner product with the row of -0)
    g, x, q = edge_graph(IP, False)
    assert np.isnan(orc.dist(x[30], q[0], IP)) and np.isnan(orc.dist(x[31], q[2], IP)) and np.isinf(orc.dist(x[32], q[0], IP))
    d0 = orc.dist(x[200], q[2], IP)
    assert d0 == 0.0 and np.signbit(d0) and orc.dist(x[33], q[0], IP) == 0.0
    return seen


def case_expansion_edges(be, shapes=None):
    """Case C.  Every scenario in every world it can take (host build: two worlds each, rotated, every world walked)."""
    scs = [sc for sc in edge_scenarios() if shapes is None or sc.tag[1] in shapes]
    walked = set()
    for j, sc in enumerate(scs):
        avail = sc.worlds()
        worlds = [avail[(3 * j) % len(avail)], avail[(3 * j + 4) % len(avail)]] if be.emulated else avail
        sc.run(be, worlds=worlds)
        walked |= set(worlds)
        print(f"{sc.tag}: {' '.join(worlds)}: ok", flush=True)
    if shapes is None:
        assert walked == set(WORLDS), sorted(set(WORLDS) - walked)
    return walked


CASES["expansion_edges"] = case_expansion_edges


# ---- case D: the LDS envelope of a CSR index ----------------------------------------------------------------------------------------------
def lds_bytes(info, ef, k, beam):
    """(persistent, lock-step) bytes of search_lds_checks, from the graph's own largest degrees."""
    maxnew = max(beam * int(info.max_degree0), int(info.max_degree_up), 1)
    keys = 2 * max(ef, k) + next_pow2(maxnew)
    return keys * 8 + 4 * maxnew, keys * 8


def envelope_world(emulated):
    key = ("D", emulated)
    if key not in _CACHE:
        n, d = (300 if emulated else 1200), 61
        rng = np.random.default_rng(616)
        x = rng.standard_normal((n, d)).astype(np.float32)
        q = (x[rng.integers(0, n, 3)] + 0.3 * rng.standard_normal((3, d))).astype(np.float32)
        _CACHE[key] = (layered_graph(n, d, L2, 617), x, q)
    return _CACHE[key]


def reachable_level0(g, start):
    seen, stack = {start}, [start]
    while stack:
        for v in nbr_list(g, stack.pop(), 0).tolist():
            if v not in seen:
                seen.add(v)
                stack.append(v)
    return np.array(sorted(seen), np.int64)


def case_lds_envelope(be):
    """Case D.  k = 10, beam 8.  ef_p / ef_l: the largest efSearch whose state fits 150 KiB (persistent) / 64 KiB (lock-step)."""
    from leann_amd.index import Mi355xIndex
    from oracle import oracle as orc

    g, x, q = envelope_world(be.emulated)
    k, beam, n = 10, 8, x.shape[0]
    idx = Mi355xIndex.from_csr(g)
    be.prepare(idx)
    info = idx.info
    ef_p = max(e for e in range(1, 20000) if lds_bytes(info, e, k, beam)[0] <= PERSIST_LDS)
    ef_l = max(e for e in range(1, 20000) if lds_bytes(info, e, k, beam)[1] <= LOCKSTEP_LDS)
    assert lds_bytes(info, ef_p, k, beam)[0] <= PERSIST_LDS < lds_bytes(info, ef_p + 1, k, beam)[0]
    assert lds_bytes(info, ef_l, k, beam)[1] <= LOCKSTEP_LDS < lds_bytes(info, ef_l + 1, k, beam)[1]
    assert n < ef_l < ef_l + 1 < ef_p and lds_bytes(info, ef_p + 1, k, beam)[1] > LOCKSTEP_LDS  # above ef_p neither kernel fits
    # persistent, at its limit: the oracle's result, which with ef > N is the exact top-k of everything the walk can reach
    sp = Scenario(("envelope", "persistent limit", ef_p), g, x, q, k, ef_p, beam)
    sp.run(be, worlds=("persist_wg", "persist_wave"), idx=idx)
    for i in range(q.shape[0]):
        reach = reachable_level0(g, validated_walk(sp, i)["seed0"])
        bi, bd = orc.bruteforce_topk(x[reach], q[i], k, L2)
        oi, od, _ = sp.table()
        assert np.array_equal(reach[bi[0]], oi[i]) and np.array_equal(_bits(bd[0]), _bits(od[i])), ("envelope", "brute force over the reachable set", i)
    assert len(reach) > k
    idx.set_option("persistent_table", 1)
    idx.set_option("update_variant", 0)
    idx.attach_table(x)
    assert_refused(("envelope", "table", ef_p + 1), idx, q, k, idx.make_params(ef=ef_p + 1, beam=beam, recompute=False))
    # lock-step and provider mode, at their limit and one above it
    sl = Scenario(("envelope", "lock-step limit", ef_l), g, x, q, k, ef_l, beam)
    sl.run(be, worlds=("lock_wg", "rank_wg", "memo") if be.emulated else ("lock_wg", "lock_wave", "rank_wg", "rank_wave", "memo"), idx=idx)
    fn, calls = be.provider(x, int(info.d_padded))
    idx.set_provider(fn)
    for opts, recompute in (((("persistent_table", 0),), False), ((("update_variant", 4),), False), ((), True)):
        for name, v in opts:
            idx.set_option(name, v)
        assert_refused(("envelope", opts, recompute, ef_l + 1), idx, q, k, idx.make_params(ef=ef_l + 1, beam=beam, recompute=recompute))
        idx.set_option("persistent_table", 1)
        idx.set_option("update_variant", 0)
    assert not calls  # a refused call asks the provider for nothing
    idx.set_provider(None)
    # between the limits: the stored table is served by the persistent kernel, the provider is refused; the handle is right afterwards
    mid = (ef_l + 1 + ef_p) // 2
    sm = Scenario(("envelope", "between the limits", mid), g, x, q, k, mid, beam)
    sm.run(be, worlds=("persist_wg",), idx=idx)
    idx.set_provider(fn)
    assert_refused(("envelope", "provider between the limits", mid), idx, q, k, idx.make_params(ef=mid, beam=beam, recompute=True))
    idx.set_provider(None)
    Scenario(("envelope", "after the refusals"), g, x, q, k, 48, beam).run(be, worlds=("lock_wg", "rank_wg", "persist_wg"), idx=idx)
    idx.close()
    print(f"LDS envelope: efSearch {ef_p} persistent, {ef_l} lock-step accepted, the next refused: ok", flush=True)


CASES["lds_envelope"] = case_lds_envelope


# ---- case E: dedup over several tiles -------------------------------------------------------------------------------------------------
TILE_N = 2 * UNIQ_TILE_NODES + 37
BORDER_IDS = (UNIQ_TILE_NODES - 1, UNIQ_TILE_NODES, 2 * UNIQ_TILE_NODES - 1, 2 * UNIQ_TILE_NODES, TILE_N - 1)


def tiles_world():
    """N = 2 x 131072 + 37 nodes (three tiles of the request bitmap, the last one 37 nodes = a full word and a partial one), D = 64: a ring
    plus two seeded long links per node, and the tile-border ids listed by the entry point."""
    if "E" not in _CACHE:
        rng = np.random.default_rng(8080)
        n, d = TILE_N, 64
        x = rng.standard_normal((n, d), dtype=np.float32)
        ids = np.arange(n, dtype=np.int64)
        nb = np.stack([(ids + 1) % n, (ids - 1) % n, rng.integers(0, n, n), rng.integers(0, n, n)], 1).astype(np.int32)
        deg = np.full(n, 4, np.int64)
        flat = nb.reshape(-1)
        flat = np.concatenate([np.asarray(BORDER_IDS, np.int32), flat])  # node 0 lists the border ids first, then its own four
        deg[0] += len(BORDER_IDS)
        q = (x[[7, UNIQ_TILE_NODES + 5, TILE_N - 3]] + 0.3 * rng.standard_normal((3, d))).astype(np.float32)
        _CACHE["E"] = Scenario(("tiles",), flat_csr_arrays(deg, flat, d, IP, 0), x, q, 10, 32, beam=4)
    return _CACHE["E"]


def assert_tiles_premises(sc):
    want = sc.provider(False)[3]
    tiles = [set((r // UNIQ_TILE_NODES).tolist()) for r in want]
    assert TILE_N > 2 * UNIQ_TILE_NODES and (TILE_N + 31) // 32 > 2 * 4096 and TILE_N % 32
    assert any(t == {0, 1, 2} and r.max() >= TILE_N // 32 * 32 for t, r in zip(tiles, want)), "no round asks for ids in all three tiles and in the last partial word"
    assert any(set(BORDER_IDS) <= set(r.tolist()) for r in want)
    assert sum(len(t) > 1 for t in tiles) >= 3  # ranks cross a tile border in several rounds


def case_dedup_tiles(be):
    """Case E.  Provider mode with and without the memo: request lists equal the oracle's round by round.  Then a hub cache that holds the
    tile-border ids: same results, those ids never reach the provider, every other id of the oracle's lists does."""
    from leann_amd.index import Mi355xIndex

    sc = tiles_world()
    assert_tiles_premises(sc)
    idx = Mi355xIndex.from_csr(sc.g)
    be.prepare(idx)
    sc.run(be, worlds=("rank_wg", "memo") if be.emulated else ("rank_wg", "rank_wave", "memo", "identity"), idx=idx)
    hub = np.asarray(BORDER_IDS, np.int32)
    rows = np.zeros((len(hub), int(idx.info.d_padded)), np.float32)
    rows[:, : sc.x.shape[1]] = sc.x[hub]
    be.set_hub_cache(idx, hub, rows)
    fn, calls = be.provider(sc.x, int(idx.info.d_padded))
    idx.set_provider(fn)
    idx.set_option("update_variant", 4)
    exp = sc.provider(False)
    check_result(sc.tag + ("hub cache",), idx.search(sc.q, sc.k, sc.params(idx, True, False)), idx.stats(), exp[:3])
    want = [r[~np.isin(r, hub)] for r in exp[3]]
    check_requests(sc.tag + ("hub cache",), calls, [r for r in want if len(r)])
    assert sum(len(r) for r in want) < sum(len(r) for r in exp[3])
    idx.close()
    print("dedup over three tiles, memo, hub cache on the tile borders: ok", flush=True)


CASES["dedup_tiles"] = case_dedup_tiles


# ---- case F: sizes whose products overflow 32 bits ------------------------------------------------------------------------------------------
def case_overflow_refusals(be):
    """Case F.  batch_size and beam_size whose sums and products with a degree pass 2^31 (or merely the LDS) are LM_EINVAL before anything
    is allocated or launched: outputs untouched, the handle serves the next call; the largest batch_size that fits, and the one below, still
    equal the oracle."""
    from leann_amd.index import Mi355xIndex

    g, x, q = envelope_world(True)
    k, ef = 10, 64
    idx = Mi355xIndex.from_csr(g)
    be.prepare(idx)
    idx.attach_table(x)
    fn, calls = be.provider(x, int(idx.info.d_padded))
    idx.set_provider(fn)
    deg0 = int(idx.info.max_degree0)
    assert int(idx.info.max_degree_up) <= deg0 and deg0 > 1
    wrap_beam = (1 << 31) // deg0 + 1
    assert wrap_beam * deg0 >= 1 << 31 and wrap_beam < (1 << 31) - 1
    bad = [dict(batch_size=(1 << 31) - 1), dict(batch_size=1_000_000), dict(beam=(1 << 31) - 1), dict(beam=wrap_beam), dict(beam=(1 << 31) - 1, batch_size=(1 << 31) - 1)]
    for kw in bad:
        for recompute in (False, True):
            assert_refused(("overflow", kw, recompute), idx, q, k, idx.make_params(ef=ef, recompute=recompute, **kw))
    assert not calls
    idx.set_provider(None)
    # the largest batch_size the lock-step LDS holds: P(batch_size - 1 + deg0) = 4096 beside 2 x 64 pool keys
    fit = 4096 + 1 - deg0
    assert (2 * ef + next_pow2(fit - 1 + deg0)) * 8 <= LOCKSTEP_LDS < (2 * ef + next_pow2(fit + deg0)) * 8
    for bs in (fit, fit - 1):
        Scenario(("overflow", "batch_size that fits", bs), g, x, q, k, ef, batch_size=bs).run(be, worlds=("lock_wg", "rank_wg"), idx=idx)
    idx.set_provider(fn)
    for recompute in (False, True):
        assert_refused(("overflow", "batch_size one above", recompute), idx, q, k, idx.make_params(ef=ef, recompute=recompute, batch_size=fit + 1))
    idx.set_provider(None)
    Scenario(("overflow", "after the refusals"), g, x, q, k, ef, beam=2).run(be, worlds=("persist_wg", "lock_wg", "memo"), idx=idx)
    idx.close()
    print("overflowing batch_size / beam_size refused, outputs untouched, handle usable: ok", flush=True)


CASES["overflow_refusals"] = case_overflow_refusals


if __name__ == "__main__":
    sys.path.insert(0, str(ROOT))
    _load(sys.argv[1])
    import time

    import torch

    torch.set_num_threads(1)
    for arg in (sys.argv[2:] or list(CASES)):
        name, _, sub = arg.partition(":")
        t0 = time.time()
        if name == "every_form":
            CASES[name](HostBackend(), widths=tuple(int(v) for v in sub.split(",")) if sub else None)
        elif name == "expansion_edges":
            CASES[name](HostBackend(), shapes=tuple(sub.split(",")) if sub else None)
        else:
            CASES[name](HostBackend())
        print(f"[case {arg}: {time.time() - t0:.1f} s]", flush=True)
    print("ALL CASES OK")
