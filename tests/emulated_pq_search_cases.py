"""Edge cases of the DiskANN-style search (csrc/lm_pq_impl.h: k_pq_traverse, k_pq_rerank, k_pq_mark, pq_search_pass) against the two
oracles (oracle/lm_oracle_pq.c, oracle/lm_oracle_diskann.c): labels, distance BITS and the ndis / nexpand / nrounds counts, no
tolerance anywhere.  The shapes and inputs live here; tests/test_gpu_pq_search_edges.py runs them on the MI355X (all three workgroup
widths), tests/test_pq_search_edges.py runs them against the host build of the library (tests/hip_emul/build_emul_lib.py):
    python -m tests.emulated_pq_search_cases <path/to/libleann_mi355x_emul.so> [case ...]
The host build runs 256 threads per query (one OS thread per lane) and smaller corpora: case A N = 200 instead of 600, case D 3000
nodes of degree 48 / 64 instead of 4000 / 12000 of degree 128 / 64 (the premises are asserted against 4 x 256 neighbour slots per
group instead of 4 x 1024), case E N = 400 instead of 1500.  GPU only: the 1024- and 512-thread widths of every case, case D at
its full size, case G (4100 queries = two passes, the workspace shared with the HNSW search, the device entry point).

Case D as the issue words it cannot hold: 64 pops x 128 neighbours are 8192 slots, but a graph of 4000 nodes has fewer than 4096
fresh ones to give.  The 4000-node graph therefore asserts what it can reach (more than one group of neighbour SLOTS, more than
PQ_RANK_SORT_MAX fresh nodes into a list that is not full) and a 12000-node graph of the same degree asserts the fresh set > 4096."""
import ctypes as C
import re
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
PQ_IMPL = ROOT / "leann_amd" / "csrc" / "lm_pq_impl.h"
LDS_LIMIT = 158 * 1024           # pq_search_pass: shmem > 158 * 1024 is LM_EINVAL
EP = 4                           # k_pq_traverse: workgroup passes of neighbour slots in flight at a time
PQ_RANK_SORT_MAX = 512           # survivors of a hop above which they are sorted, not counted into place
ORACLE_MAX_POPS, ORACLE_MAX_NEW = 64, 8192  # orc_pq_search stops collecting at 1024 pops / 8192 new keys per round, silently
IP, L2 = 0, 1
METRIC_NAME = {IP: "mips", L2: "l2"}
CASES = {}
_CACHE = {}


def _load(lib_path: str):
    from leann_amd import _lib

    _lib.LIB_PATH = Path(lib_path)
    _lib._lib = None
    return _lib.load()


# ---- the two worlds ------------------------------------------------------------------------------------------------------------
class HostBackend:
    """The host build of the library: 'device' pointers are host pointers, one workgroup width."""

    emulated = True
    widths = (256,)

    def prepare(self, idx):
        idx.set_option("pq_threads", 256)

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


class GpuBackend:
    """The MI355X: the default width first, then the two others."""

    emulated = False
    widths = (1024, 512, 256)

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


# ---- comparison ----------------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _eq(tag, got, exp):
    (gi, gd), (ei, ed) = got, exp
    nl, nd = int((gi != ei).sum()), int((_bits(gd) != _bits(ed)).sum())
    assert nl == 0 and nd == 0, (tag, f"{nl} labels and {nd} distance words of {gi.size} differ")


def _counts(tag, st, ost):
    got = (int(st["ndis"]), int(st["nexpand"]), int(st["nrounds"]))
    assert got == (ost["n_adc"], ost["n_expand"], ost["n_rounds"]), (tag, got, ost)


def flat_csr(adj, d, metric, entry_point):
    """A single-level graph in the layout of leann_amd.pq.flat_graph from per-node neighbour lists, kept exactly as given
    (duplicates, self loops, empty lists)."""
    from leann_amd.csr_format import HnswCsr

    n = len(adj)
    deg = np.array([len(a) for a in adj], np.int64)
    cs = np.cumsum(deg)
    level_ptr = np.zeros(2 * n, np.uint64)
    level_ptr[0::2] = cs - deg
    level_ptr[1::2] = cs
    nb = np.concatenate([np.asarray(a, np.int32).reshape(-1) for a in adj] + [np.zeros(0, np.int32)]).astype(np.int32)
    assert nb.size == 0 or (0 <= nb.min() and nb.max() < n)  # the kernel dereferences every id
    return HnswCsr(d=d, ntotal=n, metric_type=metric, levels=np.ones(n, np.int32), level_ptr=level_ptr,
                   node_offsets=np.arange(n + 1, dtype=np.uint64) * 2, neighbors=nb, entry_point=entry_point, max_level=0)


def _medoid(x):
    return int(np.argmin(((x - x.mean(0)) ** 2).sum(1)))


def _knn_graph(x, deg, metric):
    """Exact kNN lists (distinct, no self loop), entered at the medoid."""
    s = x.astype(np.float64) @ x.astype(np.float64).T
    if metric == L2:
        n2 = (x.astype(np.float64) ** 2).sum(1)
        s = 2 * s - n2[:, None] - n2[None, :]
    np.fill_diagonal(s, -np.inf)
    nb = np.argsort(-s, axis=1, kind="stable")[:, :deg]
    return flat_csr(list(nb), x.shape[1], metric, _medoid(x))


def _random_regular(n, deg, seed):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        c = rng.choice(n - 1, deg, replace=False)
        out.append(np.where(c >= i, c + 1, c).astype(np.int32))  # distinct, never i itself
    return out


def _uniform_pq(x, m, iters=4):
    import torch

    from leann_amd.pq import encode_pq, train_pq

    xt = torch.from_numpy(x)
    cb = train_pq(xt, m, iters=iters, seed=0)
    return cb.numpy(), encode_pq(xt, cb).numpy()


def _numpy_codes(x, cb_flat, off):
    """argmin over float64 squared distances per chunk (an empty chunk gets code 0)."""
    m = len(off) - 1
    codes = np.zeros((x.shape[0], m), np.uint8)
    for j in range(m):
        lo, hi = int(off[j]), int(off[j + 1])
        if hi > lo:
            c = cb_flat[256 * lo : 256 * hi].reshape(256, hi - lo).astype(np.float64)
            d2 = ((x[:, None, lo:hi].astype(np.float64) - c[None]) ** 2).sum(-1)
            codes[:, j] = d2.argmin(1)
    return codes


def _chunked_pq(x, off, seed):
    """Flat per-chunk codebooks in the layout of lm_pq_attach_chunked: 256 centroids per chunk drawn from the rows and moved by one
    Lloyd step in numpy, codes by argmin."""
    rng = np.random.default_rng(seed)
    n = x.shape[0]
    flat = np.zeros(256 * int(off[-1]), np.float32)
    pick = rng.permutation(n)[:256] if n >= 256 else np.arange(256) % n
    for j in range(len(off) - 1):
        lo, hi = int(off[j]), int(off[j + 1])
        flat[256 * lo : 256 * hi] = x[pick, lo:hi].reshape(-1)
    codes = _numpy_codes(x, flat, off)
    for j in range(len(off) - 1):
        lo, hi = int(off[j]), int(off[j + 1])
        blk = flat[256 * lo : 256 * hi].reshape(256, hi - lo)
        for c in np.unique(codes[:, j]) if hi > lo else ():
            blk[c] = x[codes[:, j] == c, lo:hi].mean(0)
    return flat, _numpy_codes(x, flat, off)


def open_index(be, g, cb, codes, off=None):
    from leann_amd.index import Mi355xIndex

    idx = Mi355xIndex.from_csr(g)
    be.prepare(idx)
    idx.attach_pq(cb, codes, off)
    return idx


def assert_oracle_premises(idx, W):
    """orc_pq_search stops collecting pops and new keys at fixed sizes without saying so: every case stays inside them."""
    assert 1 <= W <= ORACLE_MAX_POPS and W * int(idx.info.max_degree0) <= ORACLE_MAX_NEW, (W, int(idx.info.max_degree0))


def run_modes(be, tag, idx, og, x, cb, codes, off, q, k, L, W, modes, widths=None):
    """One (graph, quantiser, query batch, k, L, W) through the named modes on an open handle:
    pq = PQ order with counts (skip_search_reorder) at every width; deferred = one provider call over the sorted union of the final
    lists; table / f16 = stored fp32 / fp16 rows (the oracle sees the fp16 values widened)."""
    from oracle import oracle as orc

    assert_oracle_premises(idx, W)
    kw = dict(L=L, W=W, chunk_off=off)
    if "pq" in modes:
        exp = orc.pq_search(og, cb, codes, q, k, skip_search_reorder=True, **kw)
        for t in widths or be.widths:
            idx.set_option("pq_threads", t)
            got = idx.pq_search(q, k, idx.make_pq_params(L, W, skip_search_reorder=True))
            _eq((tag, "pq order", t), got, exp[:2])
            _counts((tag, "pq order", t), idx.stats(), exp[2])
        idx.set_option("pq_threads", be.widths[0])
    if "deferred" in modes:
        fn, calls = be.provider(x, int(idx.info.d_padded))
        idx.set_provider(fn)
        exp = orc.pq_search(og, cb, codes, q, k, provider=lambda ids: x[ids], use_deferred_fetch=True, **kw)
        got = idx.pq_search(q, k, idx.make_pq_params(L, W, use_deferred_fetch=True))
        idx.set_provider(None)
        assert len(calls) == 1 and np.all(np.diff(calls[0]) > 0) and len(calls[0]) == exp[2]["n_rerank_unique"], (tag, len(calls), exp[2])
        _eq((tag, "deferred"), got, exp[:2])
        _counts((tag, "deferred"), idx.stats(), exp[2])
    for mode, tab in (("table", x), ("f16", x.astype(np.float16))):
        if mode in modes:
            idx.attach_table(tab)
            exp = orc.pq_search(og, cb, codes, q, k, table=tab.astype(np.float32), **kw)
            got = idx.pq_search(q, k, idx.make_pq_params(L, W))
            _eq((tag, mode), got, exp[:2])
            _counts((tag, mode), idx.stats(), exp[2])


# ---- case A: every ADC / LUT / rerank instantiation -------------------------------------------------------------------------------
CHUNKS_16 = [4, 4, 4, 4, 7, 0, 4, 1, 4, 4, 9, 4, 0, 4, 4, 4]                                              # ends at 61 < 70
CHUNKS_32 = [4, 4, 4, 4, 5, 0, 4, 13, 4, 1, 4, 4, 4, 4, 5, 4, 0, 4, 4, 4, 13, 4, 1, 4, 4, 4, 4, 4, 5, 4, 0, 4]  # ends at 131 < 140
LAYOUTS = [
    # (name, m, D, chunk lengths or None for uniform D / m)
    ("m16-d64", 16, 64, None), ("m32-d128", 32, 128, None), ("m48-d192", 48, 192, None), ("m64-d256", 64, 256, None),
    ("m96-d384", 96, 384, None), ("m128-d512", 128, 512, None),       # adc1's compiled forms, sub-vector length 4
    ("m80-d320", 80, 320, None),                                       # generic 16-byte loop
    ("m4-d24", 4, 24, None), ("m8-d64", 8, 64, None), ("m20-d100", 20, 100, None), ("m12-d36", 12, 36, None),  # dword loop, short tables
    ("m64-d768", 64, 768, None), ("m128-d1024", 128, 1024, None),      # rerank widths 768 and 1024
    ("m16-d70-chunked", 16, 70, CHUNKS_16), ("m32-d140-chunked", 32, 140, CHUNKS_32),
]


def layout_offsets(lay):
    _, m, d, lens = lay
    lens = [d // m] * m if lens is None else lens
    assert len(lens) == m and sum(lens) <= d
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def layout_coverage():
    """What LAYOUTS reaches, beside what the kernel source compiles in (read from csrc/lm_pq_impl.h)."""
    src = PQ_IMPL.read_text()
    switch = {int(v) for v in re.findall(r"case (\d+): return adc_pieces", src)}
    widths = {64 * int(v) for v in re.findall(r"CASER\((\d+)\)", src)}
    ms = {lay[1] for lay in LAYOUTS}
    lens = set()
    for lay in LAYOUTS:
        lens |= set(np.diff(layout_offsets(lay)).tolist())
    return dict(switch=switch, widths=widths, ms=ms, lens=lens, padded={(lay[2] + 63) // 64 * 64 for lay in LAYOUTS})


def assert_layouts_cover_every_instantiation():
    c = layout_coverage()
    assert c["switch"] == {16, 32, 48, 64, 96, 128} and c["switch"] <= c["ms"]              # every case label of adc1's switch
    assert any(m % 16 == 0 and m not in c["switch"] for m in c["ms"])                        # generic 16-byte loop
    assert any(m % 16 != 0 for m in c["ms"])                                                 # dword loop
    assert any(m * 256 < 4 * 1024 for m in c["ms"])                                          # a table shorter than one group of entries
    assert c["widths"] == {64, 128, 192, 256, 320, 384, 512, 768, 1024} and c["widths"] <= c["padded"]  # all nine k_pq_rerank widths
    assert 0 in c["lens"] and any(v % 4 and v > 4 for v in c["lens"])                        # empty chunk; 4-unrolled loop with a remainder
    for nth in (256, 512, 1024):  # chunked: some thread's four entries (NTH apart) mix length-4 chunks with other lengths, empty ones included
        for lay in LAYOUTS:
            if lay[3] is not None:
                ln, ne = np.diff(layout_offsets(lay)), lay[1] * 256
                groups = [[int(ln[min(e0 + u * nth, ne - 1) >> 8]) for u in range(4)] for e0 in range(0, ne, 256) if e0 % (4 * nth) < nth]
                assert any(4 in gp and any(v != 4 for v in gp) for gp in groups), (lay[0], nth)
                assert any(4 in gp and 0 in gp for gp in groups), (lay[0], nth)


def _layout_inputs(lay, metric, emulated):
    from leann_amd.hnsw_builder import build_hnsw
    from leann_amd.pq import flat_graph
    from tests.util import clustered, queries_near

    name, m, d, lens = lay
    n = 200 if emulated else 600
    key = ("A", n, d, metric)
    if key not in _CACHE:
        x = clustered(n, d, 100 + d)
        _CACHE[key] = (x, flat_graph(build_hnsw(x, METRIC_NAME[metric], M=8, ef_construction=40), x), queries_near(x, 9, 200 + d))
    x, g, q = _CACHE[key]
    key = ("A-pq", n, name)
    if key not in _CACHE:
        off = None if lens is None else layout_offsets(lay)
        _CACHE[key] = (_uniform_pq(x, m) if lens is None else _chunked_pq(x, off, 300 + d)) + (off,)
    cb, codes, off = _CACHE[key]
    return x, g, q, cb, codes, off


def case_every_instantiation(be, layouts=None):
    """Case A.  9 queries, k = 10, L = 40, W = 4, both metrics, every layout of LAYOUTS in every mode."""
    from tests.util import oracle_graph

    for lay in LAYOUTS:
        if layouts is not None and lay[0] not in layouts:
            continue
        for metric in (IP, L2):
            x, g, q, cb, codes, off = _layout_inputs(lay, metric, be.emulated)
            idx = open_index(be, g, cb, codes, off)
            assert int(idx.info.d_padded) == (lay[2] + 63) // 64 * 64
            run_modes(be, (lay[0], METRIC_NAME[metric]), idx, oracle_graph(g, lay[2]), x, cb, codes, off, q, 10, 40, 4, ("pq", "deferred", "table", "f16"))
            idx.close()
        print(f"layout {lay[0]}: ok", flush=True)


CASES["every_instantiation"] = case_every_instantiation


# ---- case B: degenerate graphs -----------------------------------------------------------------------------------------------------
def degenerate_inputs():
    """24 seeded single-level graphs: degrees 0..6 drawn WITH replacement from all nodes (duplicates inside a list, self loops), n
    around the multiples of 32 (the visited bitmap's words), an entry point without neighbours, L = 1, L > n, k > L, W = 64."""
    forced_n = [1, 2, 31, 32, 33, 63, 64, 65]
    out = []
    for s in range(24):
        rng = np.random.default_rng(7000 + s)
        n = forced_n[s] if s < len(forced_n) else int(rng.integers(1, 70))
        adj = [rng.integers(0, n, int(rng.integers(0, 7))).astype(np.int32) for _ in range(n)]
        ep = int(rng.integers(0, n))
        if s in (0, 3, 9, 14):
            adj[ep] = np.zeros(0, np.int32)
        L, W = int(rng.integers(1, n + 6)), int(rng.integers(1, 65))
        L = {2: 1, 6: n + 5}.get(s, L)
        W = {4: 64, 2: 64}.get(s, W)
        k = L + 3 if s in (5, 11) else int(rng.integers(1, L + 4))
        x = rng.standard_normal((n, 32)).astype(np.float32)
        cb = (0.7 * rng.standard_normal((8, 256, 4))).astype(np.float32)
        codes = _numpy_codes(x, cb.reshape(-1), np.arange(9) * 4)
        q = rng.standard_normal((3, 32)).astype(np.float32)
        out.append(dict(seed=s, n=n, adj=adj, ep=ep, metric=s % 2, L=L, W=W, k=k, x=x, cb=cb, codes=codes, q=q))
    return out


def _reachable(adj, ep):
    seen, stack = {ep}, [ep]
    while stack:
        for v in adj[stack.pop()].tolist():
            if v not in seen:
                seen.add(v)
                stack.append(v)
    return seen


def assert_degenerate_premises(graphs):
    assert len(graphs) == 24 and {1, 2, 31, 32, 33, 63, 64, 65} <= {g["n"] for g in graphs}
    assert sum(len(g["adj"][g["ep"]]) == 0 for g in graphs) >= 2
    assert any(len(_reachable(g["adj"], g["ep"])) < g["n"] for g in graphs)
    assert any(len(np.unique(a)) < len(a) for g in graphs for a in g["adj"])                  # duplicates inside one list
    assert any(i in a.tolist() for g in graphs for i, a in enumerate(g["adj"]))               # self loops
    assert any(g["L"] == 1 for g in graphs) and any(g["L"] > g["n"] for g in graphs)
    assert any(g["W"] == 64 for g in graphs) and any(g["k"] > g["L"] for g in graphs)
    assert {g["metric"] for g in graphs} == {IP, L2}


def case_degenerate_graphs(be):
    """Case B.  Unfilled slots come back as the oracle leaves them: label -1, +inf (L2) / -inf (inner product).  Nodes without
    neighbours give hops that gather nothing: before k_pq_traverse passed a barrier of its own on such a hop, the host build of this
    case stopped making progress in 3 of 12 runs (wave 0 selected the next pops while other waves still read this hop's)."""
    from tests.util import oracle_graph

    graphs = degenerate_inputs()
    assert_degenerate_premises(graphs)
    unfilled = 0
    for gr in graphs:
        g = flat_csr(gr["adj"], 32, gr["metric"], gr["ep"])
        idx = open_index(be, g, gr["cb"], gr["codes"])
        tag = ("degenerate", gr["seed"], gr["n"], gr["L"], gr["W"], gr["k"])
        run_modes(be, tag, idx, oracle_graph(g, 32), gr["x"], gr["cb"], gr["codes"], None, gr["q"], gr["k"], gr["L"], gr["W"], ("pq", "table", "deferred"))
        l, d = idx.pq_search(gr["q"], gr["k"], idx.make_pq_params(gr["L"], gr["W"]))
        assert np.all(np.isinf(d[l < 0])) and np.all((d[l < 0] > 0) == (gr["metric"] == L2)), tag
        unfilled += int((l < 0).sum())
        idx.close()
    assert unfilled > 0
    print(f"degenerate graphs x{len(graphs)}: ok ({unfilled} unfilled slots)", flush=True)


CASES["degenerate_graphs"] = case_degenerate_graphs


# ---- case C: ties and special values -----------------------------------------------------------------------------------------------
def ties_inputs(metric):
    from tests.util import clustered

    key = ("C", metric)
    if key not in _CACHE:
        rng = np.random.default_rng(4242)
        base = clustered(250, 32, 77)
        x = np.ascontiguousarray(base[np.arange(500) % 250])      # every row at least twice: tied exact distances
        cb, _ = _uniform_pq(x, 8)
        rows = rng.integers(0, 256, (5, 8)).astype(np.uint8)
        codes = np.ascontiguousarray(rows[rng.integers(0, 5, 500)])  # five distinct code rows: tied ADC distances everywhere
        g = flat_csr(_random_regular(500, 10, 4243), 32, metric, 17)
        q = np.stack([base[3] + 0.05 * rng.standard_normal(32).astype(np.float32), np.zeros(32, np.float32), base[9].copy(), base[11].copy()])
        q[2, 5] = np.nan
        q[3, 20] = np.inf
        _CACHE[key] = (x, g, cb, codes, np.ascontiguousarray(q, np.float32))
    return _CACHE[key]


def case_ties_and_special_values(be):
    """Case C.  Order is (distance, id) with NaN as +inf (oracle/lm_oracle_pq.c: pk); the zero query under inner product gives zeros
    whose sign is compared too."""
    from tests.util import oracle_graph

    for metric in (IP, L2):
        x, g, cb, codes, q = ties_inputs(metric)
        assert len(np.unique(codes, axis=0)) == 5 and min(np.unique(x, axis=0, return_counts=True)[1]) >= 2
        idx = open_index(be, g, cb, codes)
        run_modes(be, ("ties", METRIC_NAME[metric]), idx, oracle_graph(g, 32), x, cb, codes, None, q, 30, 30, 8, ("pq", "table", "deferred"))
        idx.close()
    print("ties, zero query, NaN, inf: ok", flush=True)


CASES["ties_and_special_values"] = case_ties_and_special_values


# ---- case D: wide hops -------------------------------------------------------------------------------------------------------------
def wide_hop_inputs(n, deg, seed):
    from tests.util import clustered, queries_near

    key = ("D", n, deg, seed)
    if key not in _CACHE:
        x = clustered(n, 64, seed)
        cb, codes = _uniform_pq(x, 16, iters=3)
        _CACHE[key] = (x, _random_regular(n, deg, seed + 1), cb, codes, queries_near(x, 3, seed + 2))
    return _CACHE[key]


def second_hop(adj, ep, cb, codes, q, metric, W):
    """From the graph and the oracle's ADC distances alone: the neighbour slots and the fresh nodes of the SECOND hop of a search
    whose list (1 + deg(ep) entries after the first hop) is not full."""
    from oracle import oracle as orc

    first = np.asarray(adj[ep])
    _, adc = orc.pq_lut_adc(cb, codes, q, metric, first)
    pops = first[np.lexsort((first, adc))][:W]
    slots = np.concatenate([adj[int(p)] for p in pops])
    fresh = np.setdiff1d(np.unique(slots), np.concatenate([[ep], first]))
    return len(pops), slots.size, fresh.size


def case_wide_hops(be):
    """Case D.  W = 64, D = 64, m = 16, every node with `deg` distinct random neighbours; L = 2048 (emulated 1024: not full after the
    first hop, so the second hop keeps every fresh node and sorts them with no threshold) and L = 64."""
    from tests.util import oracle_graph

    group = EP * max(be.widths)
    big_l = 1024 if be.emulated else 2048
    # (n, degree, what the second hop must be)
    shapes = [(3000, 48, "fresh"), (3000, 64, "exact")] if be.emulated else [(4000, 128, "slots"), (12000, 128, "fresh"), (4000, 64, "exact")]
    for n, deg, kind in shapes:
        x, adj, cb, codes, q = wide_hop_inputs(n, deg, 900 + deg)
        g = flat_csr(adj, 64, L2, 5)
        assert 1 + deg < big_l  # the list is not full when the second hop is merged
        for qi in range(q.shape[0]):
            npop, slots, fresh = second_hop(adj, 5, cb, codes, q[qi], L2, 64)
            if kind == "exact":
                assert npop == 64 and slots == 64 * 64 and slots % group == 0, (npop, slots)  # whole groups, no tail: 1 at 1024 threads, 4 at 256
            elif kind == "slots":
                assert slots > group and fresh > PQ_RANK_SORT_MAX, (slots, fresh)
            else:
                assert slots > group and fresh > group and fresh > PQ_RANK_SORT_MAX, (slots, fresh)
        idx = open_index(be, g, cb, codes)
        og = oracle_graph(g, 64)
        for L in (big_l, 64):
            run_modes(be, ("wide hops", n, deg, L), idx, og, x, cb, codes, None, q, 10, L, 64, ("pq", "table"))
        idx.close()
        print(f"wide hops n={n} degree={deg} ({kind}): ok", flush=True)


CASES["wide_hops"] = case_wide_hops


# ---- case E: the LDS envelope ------------------------------------------------------------------------------------------------------
def next_pow2(v):
    p = 1
    while p < v:
        p <<= 1
    return p


def lds_bytes(info, m, L, W):
    """pq_search_pass's dynamic LDS: table + list + merge output + new keys (padded to a power of two) + new ids."""
    new = W * int(info.max_degree0)
    return m * 1024 + 16 * L + 8 * next_pow2(new) + 4 * new


def envelope_inputs(n):
    from tests.util import clustered, queries_near

    key = ("E", n)
    if key not in _CACHE:
        x = clustered(n, 384, 31, n_centers=32)
        cb, codes = _uniform_pq(x, 96, iters=3)
        _CACHE[key] = (x, _knn_graph(x, 64, IP), cb, codes, queries_near(x, 4, 32))
    return _CACHE[key]


def case_lds_envelope(be):
    """Case E.  D = 384, m = 96, degree 64, W = 64: L = 512 fits (155648 bytes) and equals the oracle in every mode; L = 1024 (163840
    bytes) is refused with a ValueError that names the LDS; the next L = 512 search on the same handle is right again."""
    from tests.util import oracle_graph

    x, g, cb, codes, q = envelope_inputs(400 if be.emulated else 1500)
    idx = open_index(be, g, cb, codes)
    assert int(idx.info.max_degree0) == 64
    fits, over = lds_bytes(idx.info, 96, 512, 64), lds_bytes(idx.info, 96, 1024, 64)
    assert (fits, over) == (155648, 163840) and fits <= LDS_LIMIT < over
    og = oracle_graph(g, 384)
    run_modes(be, ("envelope", 512), idx, og, x, cb, codes, None, q, 10, 512, 64, ("pq", "deferred", "table", "f16"))
    for prm in (idx.make_pq_params(1024, 64, skip_search_reorder=True), idx.make_pq_params(1024, 64)):
        try:
            idx.pq_search(q, 10, prm)
        except ValueError as ex:
            assert "LDS" in str(ex), str(ex)
        else:
            raise AssertionError("L = 1024 was accepted although its state does not fit the LDS")
    run_modes(be, ("envelope", 512, "after the refusal"), idx, og, x, cb, codes, None, q, 10, 512, 64, ("pq", "table"))
    idx.close()
    print(f"LDS envelope: {fits} bytes accepted, {over} refused: ok", flush=True)


CASES["lds_envelope"] = case_lds_envelope


# ---- case F: expanded-set overflow -------------------------------------------------------------------------------------------------
def expanded_expectation(og, cb, codes, q, k, L, W, x):
    """pq_rerank_expanded per query, decided by the oracle one query at a time: a query that expands more than 4 L nodes gets the
    final-list rerank (orc.pq_search with a table), every other the rerank of all expanded nodes (the DiskANN transcription).
    Returns (labels, distances, over-the-cap mask)."""
    from oracle import oracle as orc

    assert k <= L  # exp_cap = 4 max(L, k)
    nexp = np.array([orc.pq_search(og, cb, codes, q[i : i + 1], k, L=L, W=W, skip_search_reorder=True)[2]["n_expand"] for i in range(q.shape[0])])
    over = nexp > 4 * L
    fi, fd, _ = orc.pq_search(og, cb, codes, q, k, L=L, W=W, table=x)
    di, dd, _ = orc.diskann_search(og, cb, codes, q, k, L=L, W=W, table=x, rerank_final_list_only=True)
    assert np.array_equal(fi, di) and np.array_equal(_bits(fd), _bits(dd))  # the two oracles agree on the fallback
    ui, ud, _ = orc.diskann_search(og, cb, codes, q, k, L=L, W=W, table=x, rerank_final_list_only=False)
    return np.where(over[:, None], fi, ui), np.where(over[:, None], fd, ud), over


def overflow_inputs():
    """(a) a chain along one direction (node i links i - 1, i + 1, i + 2), entered at node 0: a query near the far end walks the whole
    chain, a query near the entry stops after a few nodes; (b) a 12 x 12 lattice in a plane
    (4-neighbourhood), entered at a corner, with queries near that corner and far from it."""
    if "F" not in _CACHE:
        rng = np.random.default_rng(555)
        n = 80
        u = rng.standard_normal(32).astype(np.float32)
        u /= np.linalg.norm(u)
        x = (0.25 * np.arange(n, dtype=np.float32)[:, None] * u[None] + 0.01 * rng.standard_normal((n, 32))).astype(np.float32)
        adj = [np.array([j for j in (i - 1, i + 1, i + 2) if 0 <= j < n], np.int32) for i in range(n)]
        q = np.ascontiguousarray(x[[0, 2, 5, 20, 40, 79, 1, 60]] + 0.005 * rng.standard_normal((8, 32)).astype(np.float32), np.float32)
        chain = (x, flat_csr(adj, 32, L2, 0), _uniform_pq(x, 8), q)
        side = 12
        v = rng.standard_normal(32).astype(np.float32)
        v -= (v @ u) * u
        v /= np.linalg.norm(v)
        ab = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2).astype(np.float32)
        y = (0.3 * (ab[:, :1] * u[None] + ab[:, 1:] * v[None]) + 0.01 * rng.standard_normal((side * side, 32))).astype(np.float32)
        adj = [np.array([a2 * side + b2 for a2, b2 in ((a - 1, b), (a + 1, b), (a, b - 1), (a, b + 1)) if 0 <= a2 < side and 0 <= b2 < side], np.int32)
               for a in range(side) for b in range(side)]
        cells = [(0, 0), (1, 1), (0, 2), (2, 0), (11, 11), (6, 9), (11, 0), (8, 8)]
        qy = np.ascontiguousarray(y[[a * side + b for a, b in cells]] + 0.005 * rng.standard_normal((8, 32)).astype(np.float32), np.float32)
        _CACHE["F"] = [("chain", chain, [(2, 1, 2), (3, 1, 3), (4, 2, 3)]), ("lattice", (y, flat_csr(adj, 32, L2, 0), _uniform_pq(y, 8), qy), [(2, 1, 2), (4, 2, 4)])]
    return _CACHE["F"]


def case_expanded_overflow(be):
    """Case F.  The branch `exp_cap > 0 && nexp > exp_cap`: the query falls back to its final list and pq_rerank_overflow counts it."""
    from oracle import oracle as orc
    from tests.util import oracle_graph

    for name, (x, g, (cb, codes), q), configs in overflow_inputs():
        og = oracle_graph(g, 32)
        idx = open_index(be, g, cb, codes)
        idx.attach_table(x)
        for L, W, k in configs:
            assert_oracle_premises(idx, W)
            wi, wd, over = expanded_expectation(og, cb, codes, q, k, L, W, x)
            nover = int(over.sum())
            assert 0 < nover < q.shape[0], (name, L, W, over)  # both kinds of query occur
            tag = ("overflow", name, L, W, k)
            idx.set_option("pq_rerank_expanded", 1)
            assert idx.get_option("pq_rerank_overflow") == 0
            for rep in (1, 2):  # through the table, twice: the counter adds up
                _eq(tag + ("table", rep), idx.pq_search(q, k, idx.make_pq_params(L, W)), (wi, wd))
                assert idx.get_option("pq_rerank_overflow") == rep * nover, (tag, rep, idx.get_option("pq_rerank_overflow"), nover)
            idx.set_option("pq_rerank_expanded", 1)  # setting the option again resets the counter
            assert idx.get_option("pq_rerank_overflow") == 0
            fn, calls = be.provider(x, int(idx.info.d_padded))
            idx.set_provider(fn)
            got = idx.pq_search(q, k, idx.make_pq_params(L, W, use_deferred_fetch=True))
            idx.set_provider(None)
            _eq(tag + ("deferred",), got, (wi, wd))
            assert len(calls) == 1 and np.all(np.diff(calls[0]) > 0), tag
            assert idx.get_option("pq_rerank_overflow") == nover
            # no rerank follows: the PQ order comes back and nothing is counted
            pi, pd, pst = orc.pq_search(og, cb, codes, q, k, L=L, W=W, skip_search_reorder=True)
            _eq(tag + ("skip",), idx.pq_search(q, k, idx.make_pq_params(L, W, skip_search_reorder=True)), (pi, pd))
            _counts(tag + ("skip",), idx.stats(), pst)
            assert idx.get_option("pq_rerank_overflow") == nover
            idx.set_option("pq_rerank_expanded", 0)
            assert idx.get_option("pq_rerank_overflow") == 0
            print(f"expanded-set overflow {name} L={L} W={W} k={k}: {nover} of {q.shape[0]} queries over the cap: ok", flush=True)
        idx.close()


CASES["expanded_overflow"] = case_expanded_overflow


# ---- case G: passes and workspace reuse (GPU only) ------------------------------------------------------------------------------------
def case_passes_and_workspace(be):
    """Case G.  4100 queries are two passes (4096 + 4) over one workspace: rows equal the oracle's, ndis / nexpand are its sums, nrounds
    its maximum.  Then, on the same handle: 3 queries; the HNSW search at ef 24; PQ with pq_rerank_expanded (workspace ef 96); HNSW at
    ef 96; PQ with the option off -- each against its oracle.  Host and device entry points return the same bits."""
    import torch

    from leann_amd.hnsw_builder import build_hnsw
    from leann_amd.pq import flat_graph
    from oracle import oracle as orc
    from tests.util import clustered, oracle_graph, queries_near

    assert not be.emulated
    x = clustered(300, 32, 21)
    g = flat_graph(build_hnsw(x, "mips", M=6, ef_construction=30), x)
    cb, codes = _uniform_pq(x, 8)
    og = oracle_graph(g, 32)
    q = queries_near(x, 4100, 22)
    k, L, W = 5, 24, 3
    idx = open_index(be, g, cb, codes)
    assert_oracle_premises(idx, W)
    idx.attach_table(x)

    def pq_both_entries(tag, qq, prm, exp, ost=None):
        got = idx.pq_search(qq, k, prm)
        _eq(tag + ("host entry",), got, exp)
        if ost is not None:
            _counts(tag + ("host entry",), idx.stats(), ost)
        dl, dd = idx.pq_search_device(torch.from_numpy(qq).cuda(), k, prm)
        _eq(tag + ("device entry",), (dl.cpu().numpy(), dd.cpu().numpy()), exp)
        if ost is not None:
            _counts(tag + ("device entry",), idx.stats(), ost)

    oi, od, ost = orc.pq_search(og, cb, codes, q, k, L=L, W=W, skip_search_reorder=True)
    pq_both_entries(("passes", "pq order"), q, idx.make_pq_params(L, W, skip_search_reorder=True), (oi, od), ost)
    ti, td, tst = orc.pq_search(og, cb, codes, q, k, L=L, W=W, table=x)
    pq_both_entries(("passes", "table"), q, idx.make_pq_params(L, W), (ti, td), tst)
    q3 = np.ascontiguousarray(q[[7, 4097, 4099]])

    def pq3(tag):
        ei, ed, est = orc.pq_search(og, cb, codes, q3, k, L=L, W=W, table=x)
        pq_both_entries(tag, q3, idx.make_pq_params(L, W), (ei, ed), est)

    def hnsw(ef):
        ei, ed, est = orc.search(og, q3, k, ef=ef, beam=3, table=x)
        d, l = idx.search(q3, k, idx.make_params(ef=ef, beam=3, recompute=False))
        _eq(("workspace", "hnsw", ef), (l, d), (ei, ed))
        st = idx.stats()
        assert (int(st["ndis"]), int(st["nexpand"]), int(st["nrounds"])) == (est["ndis"], est["nexpand"], est["nrounds"]), (ef, st, est)

    pq3(("workspace", 1))
    hnsw(24)
    idx.set_option("pq_rerank_expanded", 1)
    wi, wd, over = expanded_expectation(og, cb, codes, q3, k, L, W, x)
    pq_both_entries(("workspace", 3, "expanded"), q3, idx.make_pq_params(L, W), (wi, wd))
    assert idx.get_option("pq_rerank_overflow") == 2 * int(over.sum())
    hnsw(96)
    idx.set_option("pq_rerank_expanded", 0)
    pq3(("workspace", 5))
    idx.close()
    print("two passes, workspace shared with the HNSW search, both entry points: ok", flush=True)


GPU_ONLY_CASES = {"passes_and_workspace": case_passes_and_workspace}


if __name__ == "__main__":
    sys.path.insert(0, str(ROOT))
    _load(sys.argv[1])
    import time

    import torch

    torch.set_num_threads(1)
    for name in (sys.argv[2:] or list(CASES)):
        t0 = time.time()
        CASES[name](HostBackend())
        print(f"[case {name}: {time.time() - t0:.1f} s]", flush=True)
    print("ALL CASES OK")
