"""lm_pq_batch_search_filtered (csrc/lm_pq_impl.h: k_pq_traverse<NTH, true>) against the reference composed in tests/pq_filtered_ref_util.py:
labels equal, distance BITS equal, ndis / nexpand / nrounds equal to the unfiltered call's and the reference's, nunique and the provider's
request list equal to the sorted unique union of the F lists, "filtered_allowed_evals" equal to the reference's sum of |E n allowed| -- no
tolerance anywhere.  The inputs are those of tests/emulated_pq_search_cases.py (cases A-E); tests/test_gpu_pq_filtered_search.py runs the
cases on the MI355X (all three workgroup widths), tests/test_pq_filtered_search.py against the host build of the library
(tests/hip_emul/build_emul_lib.py, a thread per lane, 256 lanes per query):
    python -m tests.emulated_pq_filtered_cases <path/to/libleann_mi355x_emul.so> [case ...]"""
import ctypes as C
import sys
from pathlib import Path

import numpy as np

from tests import emulated_pq_search_cases as pc
from tests import pq_filtered_ref_util as pr
from tests import pq_flat_ref_util as fu
from tests.emulated_pq_search_cases import GpuBackend, HostBackend, _load, open_index  # noqa: F401  (the two worlds and their providers)
from tests.pq_filtered_ref_util import FS, IP, L2

CASES = {}
LAYOUTS_A = ("m16-d64", "m96-d384", "m16-d70-chunked")
DRAW_SEED = 7  # the 50 % / 10 % / 2 % lists: rng = default_rng(7), drawn in this order as rng.random(n) < p


def draws(n):
    rng = np.random.default_rng(DRAW_SEED)
    return rng.random(n) < 0.5, rng.random(n) < 0.1, rng.random(n) < 0.02


def layout(name):
    return next(lay for lay in pc.LAYOUTS if lay[0] == name)


def raw(be, idx, device_form, q, k, prm, words=None, n=None, null=()):
    """lm_pq_batch_search_filtered (host pointers) or _device (the world's device pointers) on sentinel-filled outputs ->
    (rc, labels [n, k], distances [n, k], untouched: every element of both buffers still holds its fill)"""
    from tests.gpu_abi_util import FILL_I64

    Mm = fu.mem(be) if device_form else fu._HostMem()
    nq = q.shape[0] if n is None else n
    own = max(nq, 0) * max(k, 0)
    hq, pq = Mm.put(np.ascontiguousarray(q, np.float32))
    hw, pw = (None, None) if words is None else Mm.put(words)
    D, pD = Mm.full(own + 64, np.nan, np.float32)
    Lb, pL = Mm.full(own + 64, FILL_I64, np.int64)
    ptr = dict(x=pq, L=pL, D=pD, params=None if prm is None else C.byref(prm), idx=idx._h)
    for name in null:
        ptr[name] = None
    fn = idx._lib.lm_pq_batch_search_filtered_device if device_form else idx._lib.lm_pq_batch_search_filtered
    rc = fn(ptr["idx"], nq, ptr["x"], k, ptr["params"], pw, ptr["L"], ptr["D"])
    hD, hL = Mm.get(D), Mm.get(Lb)
    untouched = bool(np.isnan(hD).all() and (hL == FILL_I64).all())
    assert bool(np.isnan(hD[own:]).all() and (hL[own:] == FILL_I64).all()), "wrote past the n x k outputs"
    return rc, hL[:own].reshape(max(nq, 0), max(k, 0)).copy(), hD[:own].reshape(max(nq, 0), max(k, 0)).copy(), untouched


def _stats(idx):
    st = idx.stats()
    return tuple(int(st[f]) for f in ("ndis", "nexpand", "nrounds", "nunique"))


class Handle:
    """An open index, its reference, and the rows a rerank is served from."""

    def __init__(self, be, g, cb, codes, off, x):
        self.be, self.x = be, x
        self.R = pr.Reference(g, cb, codes, off)
        self.idx = open_index(be, g, cb, codes, off)
        self.mode = None

    def set_mode(self, mode):
        """pq = PQ order (skip_search_reorder), deferred = one provider call, table / f16 = stored rows -> (params factory, served rows, calls)"""
        idx = self.idx
        if mode != self.mode:
            idx.set_provider(None)
            self.calls = None
            if mode == "deferred":
                fn, self.calls = self.be.provider(self.x, int(idx.info.d_padded))
                idx.set_provider(fn)
            elif mode in ("table", "f16"):
                idx.attach_table(self.x.astype(np.float16) if mode == "f16" else self.x)
            self.mode = mode
        self.served = None if mode == "pq" else (self.x.astype(np.float16).astype(np.float32) if mode == "f16" else self.x)
        return dict(skip_search_reorder=mode == "pq", use_deferred_fetch=mode == "deferred")

    def close(self):
        self.idx.set_provider(None)
        self.idx.close()


def check(H, tag, q, k, L, W, masks, mode, stray=True, device_form=False, widths=None):
    """One unfiltered call, then one filtered call per allow-list of `masks` (None = NULL) with the same params, at every width in PQ order:
    the filtered result is the reference's, stats agree with the unfiltered call's and the reference's (invariant 2), NULL / all ones give
    lm_pq_batch_search's bits (invariant 1).  The modes must be visited in the order pq, deferred, table, f16 on one handle (an attached table
    stays).  -> per mask (expected labels, expected distances, hits per query)"""
    be, idx, R = H.be, H.idx, H.R
    kw = H.set_mode(mode)
    prm = idx.make_pq_params(L, W, **kw)
    out = []
    for t in (widths or be.widths) if mode == "pq" else (be.widths[0],):
        idx.set_option("pq_threads", t)
        log = H.calls if H.calls is not None else []
        log.clear()
        lu, du = idx.pq_search(q, k, prm)
        su = _stats(idx)
        out = []
        for mask in masks:
            log.clear()
            words = None if mask is None else pr.bitmap(mask, stray)
            rc, lf, df, _ = raw(be, idx, device_form, q, k, prm, words)
            sf, ev, reqs = _stats(idx), idx.get_option("filtered_allowed_evals"), [c.copy() for c in log]
            el, ed, eev, hits, union, est = R.expected(q, k, L, W, mask, H.served)
            good = rc == 0 and pr.same(lf, df, el, ed) and ev == eev and sf[:3] == su[:3] == est
            if mode == "deferred":
                good = good and sf[3] == len(union) and len(reqs) == (1 if len(union) else 0) and all(np.array_equal(r, union) for r in reqs)
            else:
                good = good and sf[3] == 0
            if mask is None or mask.all():
                good = good and pr.same(lf, df, lu, du) and ev == su[0]
            frac = "NULL" if mask is None else f"{int(mask.sum())}/{mask.size}"
            print(f"pq filtered {tag} {mode} threads={t} nq={q.shape[0]} k={k} L={L} W={W} allowed={frac}: {'ok' if good else 'MISMATCH'}", flush=True)
            assert good, (tag, mode, t, rc, ev, eev, su, sf, est, len(reqs), len(union), (lf != el).sum())
            out.append((el, ed, hits))
    idx.set_option("pq_threads", be.widths[0])
    return out


MODES = ("pq", "deferred", "table", "f16")


# ---- 1. modes and allow-lists ----------------------------------------------------------------------------------------------------
def case_modes_and_allow_lists(be, layouts=LAYOUTS_A):
    """Case A's inputs (n = 200 emulated, 600 on the GPU: neither a multiple of 32, stray bits set), 9 queries, k = 10, L = 40, W = 4, both
    metrics, every mode; NULL, all ones, 50 %, 10 %, 2 %, a single evaluated node, none, the entry point alone, everything but the entry point."""
    for name in layouts:
        lay = layout(name)
        for metric in (IP, L2):
            x, g, q, cb, codes, off = pc._layout_inputs(lay, metric, be.emulated)
            n = x.shape[0]
            assert n % 32 != 0
            H = Handle(be, g, cb, codes, off, x)
            pc.assert_oracle_premises(H.idx, 4)
            m50, m10, m2 = draws(n)
            ep = int(g.entry_point)
            E0 = H.R.walk(np.ascontiguousarray(q[0]), 10, 40, 4)["E"]
            one, none, only_ep = np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, bool)
            one[int(E0[E0 != ep][3])] = True
            only_ep[ep] = True
            masks = [None, np.ones(n, bool), m50, m10, m2, one, none, only_ep, ~only_ep]
            for mode in MODES:
                res = check(H, (name, pc.METRIC_NAME[metric]), q, 10, 40, 4, masks, mode)
                assert res[5][2][0] == 1 and (res[6][0] == -1).all() and (res[7][2] == 1).all() and (res[7][0][:, 0] == ep).all()
                assert not (res[8][0] == ep).any()
            H.close()
        print(f"modes and allow-lists {name}: ok", flush=True)


CASES["modes_and_allow_lists"] = case_modes_and_allow_lists


# ---- 2. the collecting threshold -------------------------------------------------------------------------------------------------
def case_collecting_threshold(be):
    """L = 8: with the 2 % and 10 % lists the walk's list is full while the allowed-only list is not -- keys above the walk's threshold must be
    kept; with the 50 % list the allowed-only list is full and its own threshold prunes.  Also k > L, and L > n."""
    lay = layout("m16-d64")
    for metric in (IP, L2):
        x, g, q, cb, codes, off = pc._layout_inputs(lay, metric, be.emulated)
        n = x.shape[0]
        H = Handle(be, g, cb, codes, off, x)
        m50, m10, m2 = draws(n)
        above = 0
        for qi in range(q.shape[0]):  # the premises, from the reference alone
            q1 = np.ascontiguousarray(q[qi])
            adc = pr._canon(H.R.adc_all(q1))
            lst = H.R.walk(q1, 8, 8, 4)["lst"]
            assert len(lst) == 8  # the walk's list is full
            for m in (m10, m2):
                F, na = H.R.flist(q1, 8, 8, 4, m)
                above += int((adc[F] > adc[lst][-1]).sum())
            F50, na50 = H.R.flist(q1, 8, 8, 4, m50)
            assert na50 > 8 and len(F50) == 8  # full: its own threshold prunes
        assert above > 0  # allowed keys worse than the walk's last entry are part of the expected result
        for mode in ("pq", "table"):
            check(H, ("threshold", pc.METRIC_NAME[metric]), q, 8, 8, 4, [m2, m10, m50], mode)
            check(H, ("threshold k > L", pc.METRIC_NAME[metric]), q, 12, 8, 4, [m10, m50], mode)
            check(H, ("threshold L > n", pc.METRIC_NAME[metric]), q[:3], 10, n + 5, 4, [None, m50], mode)
        H.close()
    print("collecting threshold: ok", flush=True)


CASES["collecting_threshold"] = case_collecting_threshold


# ---- 3. staging overflow ---------------------------------------------------------------------------------------------------------
def case_staging_overflow(be):
    """Case D's wide hops at degree 64 (W = 64, D = 64, m = 16): all allowed and 50 % allowed, L = 1024 (2048 on the GPU: the lists are not
    full when the second hop arrives) and L = 64.  From the reference alone: the second hop's allowed fresh nodes are more than FS times its
    number of passes at every width, so some pass has more than FS of them and the stage-and-merge loop runs a second round."""
    big_l = 1024 if be.emulated else 2048
    n, deg = (3000, 64) if be.emulated else (4000, 64)
    x, adj, cb, codes, q = pc.wide_hop_inputs(n, deg, 900 + deg)
    g = pc.flat_csr(adj, 64, L2, 5)
    H = Handle(be, g, cb, codes, None, x)
    pc.assert_oracle_premises(H.idx, 64)
    m50 = draws(n)[0]
    ones = np.ones(n, bool)
    for L in (big_l, 64):
        assert pr.lds_bytes_filtered(deg, 16, L, 64) <= pr.LDS_LIMIT
        for qi in range(q.shape[0]):
            hop2 = H.R.walk(np.ascontiguousarray(q[qi]), 10, L, 64)["hops"][2]
            for t in be.widths:
                passes = -(-hop2.size // t)
                assert int(m50[hop2].sum()) > FS * passes and hop2.size > FS * passes, (hop2.size, int(m50[hop2].sum()), passes)
    for L in (big_l, 64):
        for mode in ("pq", "table"):
            check(H, ("staging overflow", n, deg), q, 10, L, 64, [ones, m50], mode)
    H.close()
    print("staging overflow: ok", flush=True)


CASES["staging_overflow"] = case_staging_overflow


# ---- 4. degenerate graphs --------------------------------------------------------------------------------------------------------
def case_degenerate_graphs(be):
    """Case B's 24 graphs with a random 50 % list each: hops that gather nothing, an entry point without neighbours (allowed and not allowed),
    duplicates and self loops."""
    graphs = pc.degenerate_inputs()
    pc.assert_degenerate_premises(graphs)
    lone = [gr["seed"] for gr in graphs if len(gr["adj"][gr["ep"]]) == 0]
    assert len(lone) >= 2
    seen = set()
    for gr in graphs:
        g = pc.flat_csr(gr["adj"], 32, gr["metric"], gr["ep"])
        mask = np.random.default_rng(8000 + gr["seed"]).random(gr["n"]) < 0.5
        if gr["seed"] in lone:
            mask[gr["ep"]] = lone.index(gr["seed"]) % 2 == 0
            seen.add(bool(mask[gr["ep"]]))
        H = Handle(be, g, gr["cb"], gr["codes"], None, gr["x"])
        pc.assert_oracle_premises(H.idx, gr["W"])
        for mode in ("pq", "deferred", "table"):
            check(H, ("degenerate", gr["seed"], gr["n"]), gr["q"], gr["k"], gr["L"], gr["W"], [mask], mode)
        H.close()
    assert seen == {True, False}
    print(f"degenerate graphs x{len(graphs)}: ok", flush=True)


CASES["degenerate_graphs"] = case_degenerate_graphs


# ---- 5. ranking ------------------------------------------------------------------------------------------------------------------
def case_ranking(be):
    """Case C's ties (five distinct code rows: tied ADC distances everywhere), the zero query under inner product, NaN and inf queries, with a
    list that keeps both of two tied ids and one that drops the lower."""
    for metric in (IP, L2):
        x, g, cb, codes, q = pc.ties_inputs(metric)
        n = x.shape[0]
        H = Handle(be, g, cb, codes, None, x)
        q0 = np.ascontiguousarray(q[0])
        F, _ = H.R.flist(q0, 30, 30, 8, None)
        adc = H.R.adc_all(q0)
        a, b = int(F[0]), int(F[1])
        assert adc[a] == adc[b] and a < b  # two tied ids head the list, lower id first
        keep = draws(n)[0].copy()
        keep[[a, b]] = True
        drop = keep.copy()
        drop[a] = False
        for mode in ("pq", "deferred", "table"):
            res = check(H, ("ranking", pc.METRIC_NAME[metric]), q, 30, 30, 8, [None, keep, drop], mode)
            if mode == "pq":
                assert res[1][0][0, 0] == a and res[1][0][0, 1] == b and res[2][0][0, 0] == b
                if metric == IP:  # the zero query: every distance is -0 -> key +0 -> -0.0 comes back, ids ascending
                    hit = res[1][0][1] >= 0
                    assert hit.any() and (res[1][1][1][hit].view(np.uint32) == 0x80000000).all() and (np.diff(res[1][0][1][hit]) > 0).all()
        H.close()
    print("ranking: ties, zero query, NaN, inf: ok", flush=True)


CASES["ranking"] = case_ranking


# ---- 6. invariants ---------------------------------------------------------------------------------------------------------------
def case_invariants(be):
    """70 queries together and alone, the host and the device entry, calls in a row with different lists, lm_pq_batch_search before and
    after, "pq_rerank_expanded" (the unfiltered call keeps its expanded-set result, the filtered one ignores the option), the HNSW search on
    the same handle afterwards (the workspace is shared)."""
    from oracle import oracle as orc
    from tests.util import queries_near

    lay = layout("m16-d64")
    x, g, _, cb, codes, off = pc._layout_inputs(lay, L2, be.emulated)
    n = x.shape[0]
    q = queries_near(x, 70, 4711)
    k, L, W = 10, 40, 4
    H = Handle(be, g, cb, codes, off, x)
    idx = H.idx
    m50, m10, _ = draws(n)
    for mode in ("pq", "table"):
        prm = idx.make_pq_params(L, W, **H.set_mode(mode))
        before = idx.pq_search(q, k, prm)
        (el, ed, _), = check(H, "invariants: 70 together", q, k, L, W, [m50], mode, widths=be.widths[:1])
        for i in (0, 33, 69):  # alone: its row of the batch
            rc, l1, d1, _ = raw(be, idx, False, q[i : i + 1], k, prm, pr.bitmap(m50))
            assert rc == 0 and pr.same(l1, d1, el[i : i + 1], ed[i : i + 1]), i
        check(H, "invariants: device entry", q, k, L, W, [m50], mode, device_form=True, widths=be.widths[:1])
        for dev in (False, True):  # no state leaks from one call into the next
            check(H, f"invariants: calls in a row, device={dev}", q[:5], k, L, W, [m10, None, m50, np.zeros(n, bool), m50], mode, device_form=dev,
                  widths=be.widths[:1])
        after = idx.pq_search(q, k, prm)
        assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
    # pq_rerank_expanded: the table is attached (mode "table" came last)
    q8 = np.ascontiguousarray(q[:8])
    # (on this graph the expanded set and the final list give the same k best: the option is exercised on case F's chain below)
    # the HNSW search on the same handle, then the filtered call again
    ei, ed2, _ = orc.search(H.R.og, q8, k, ef=24, beam=3, table=x)
    d, l = idx.search(q8, k, idx.make_params(ef=24, beam=3, recompute=False))
    assert pr.same(l, d, ei, ed2)
    check(H, "invariants: after the HNSW search", q8, k, L, W, [m10], "table", widths=be.widths[:1])
    H.close()
    # "pq_rerank_expanded" on case F's chain: with the option on the unfiltered call keeps its expanded-set result (and counts the queries
    # that fall back), the filtered call ignores the option
    name, (xc, gc, (cbc, codesc), qc), _ = pc.overflow_inputs()[0]
    Lc, Wc, kc = 4, 2, 3
    Hc = Handle(be, gc, cbc, codesc, None, xc)
    mask3 = np.arange(xc.shape[0]) % 3 != 0
    for mode in ("deferred", "table"):
        prm = Hc.idx.make_pq_params(Lc, Wc, **Hc.set_mode(mode))
        wi, wd, over = pc.expanded_expectation(Hc.R.og, cbc, codesc, qc, kc, Lc, Wc, xc)
        nover = int(over.sum())
        assert 0 < nover < qc.shape[0]  # premise: the unfiltered call's expanded-set branch and its fallback both run, and the fallback is counted
        Hc.idx.set_option("pq_rerank_expanded", 1)
        for rep in range(2):  # the unfiltered call before and after the filtered ones
            got = Hc.idx.pq_search(qc, kc, prm)
            assert pr.same(got[0], got[1], wi, wd)
            assert Hc.idx.get_option("pq_rerank_overflow") == (rep + 1) * nover  # (the filtered calls in between counted nothing: they record no expanded set)
            if rep == 0:  # the filtered results are the reference's, which knows no such option
                want = [Hc.R.expected(qc, kc, Lc, Wc, m, Hc.served)[:3] for m in (None, mask3)]
                for (el, ed, _), m in zip(want, (None, mask3)):
                    if Hc.calls is not None:
                        Hc.calls.clear()
                    rc, lf, df, _ = raw(be, Hc.idx, False, qc, kc, prm, None if m is None else pr.bitmap(m))
                    assert rc == 0 and pr.same(lf, df, el, ed)
                    if mode == "deferred":  # F's rows, not the expanded sets'
                        assert len(Hc.calls) == 1 and np.array_equal(Hc.calls[0], Hc.R.expected(qc, kc, Lc, Wc, m, xc)[4])
    Hc.idx.set_option("pq_rerank_expanded", 0)
    Hc.close()
    print("invariants: ok", flush=True)


CASES["invariants"] = case_invariants


def case_two_passes(be):
    """GPU only: 4100 queries are two passes (4096 + 4) over one workspace, as case G: rows equal the reference's, the counts are its sums,
    one provider call per pass.  (41 distinct queries, each a hundred times: invariant 3 makes their rows equal.)"""
    from tests.util import queries_near

    assert not be.emulated
    lay = layout("m16-d64")
    x, g, _, cb, codes, off = pc._layout_inputs(lay, IP, False)
    q41 = queries_near(x, 41, 4712)
    q = np.ascontiguousarray(np.tile(q41, (100, 1)))
    k, L, W = 10, 40, 4
    H = Handle(be, g, cb, codes, off, x)
    idx = H.idx
    mask = draws(x.shape[0])[1]
    for mode in ("pq", "deferred", "table"):
        prm = idx.make_pq_params(L, W, **H.set_mode(mode))
        el, ed, eev, _, _, est = H.R.expected(q41, k, L, W, mask, H.served)
        if H.calls is not None:
            H.calls.clear()
        rc, lf, df, _ = raw(be, idx, mode == "table", q, k, prm, pr.bitmap(mask, True))
        st, ev = _stats(idx), idx.get_option("filtered_allowed_evals")
        assert rc == 0 and pr.same(lf, df, np.tile(el, (100, 1)), np.tile(ed, (100, 1))), mode
        assert ev == 100 * eev and st[:3] == (100 * est[0], 100 * est[1], est[2]), (mode, ev, eev, st, est)
        if mode == "deferred":
            u1 = H.R.expected(q[:4096], k, L, W, mask, H.served)[4]
            u2 = H.R.expected(q[4096:], k, L, W, mask, H.served)[4]
            assert len(H.calls) == 2 and np.array_equal(H.calls[0], u1) and np.array_equal(H.calls[1], u2) and st[3] == len(u1) + len(u2)
    H.close()
    print("two passes: ok", flush=True)


GPU_ONLY_CASES = {"two_passes": case_two_passes}


# ---- 7. the LDS envelope ---------------------------------------------------------------------------------------------------------
ENVELOPE_L = 576  # the largest L the header's rule admits at m = 96, W = 64, degree 64


def case_lds_envelope(be):
    """Case E's shape (D = 384, m = 96, degree 64, W = 64): L = 576 needs exactly 161792 bytes and is right in every mode; L = 577 is refused
    with a ValueError that names the LDS, the outputs untouched; the next L = 576 search on the same handle is right again.  L = 256, the
    shape C3 is measured on, is admitted."""
    from leann_amd import _lib

    x, g, cb, codes, q = pc.envelope_inputs(400 if be.emulated else 1500)
    H = Handle(be, g, cb, codes, None, x)
    idx = H.idx
    assert int(idx.info.max_degree0) == 64
    fits, over = pr.lds_bytes_filtered(64, 96, ENVELOPE_L, 64), pr.lds_bytes_filtered(64, 96, ENVELOPE_L + 1, 64)
    assert fits == pr.LDS_LIMIT == 161792 < over and pr.lds_bytes_filtered(64, 96, 256, 64) < pr.LDS_LIMIT
    m50 = draws(x.shape[0])[0]
    for mode in MODES:
        check(H, ("envelope", ENVELOPE_L), q, 10, ENVELOPE_L, 64, [m50, None], mode)
    for prm in (idx.make_pq_params(ENVELOPE_L + 1, 64, skip_search_reorder=True), idx.make_pq_params(ENVELOPE_L + 1, 64)):
        for dev in (False, True):
            rc, _, _, untouched = raw(be, idx, dev, q, 10, prm, pr.bitmap(m50))
            assert rc == _lib.LM_EINVAL and untouched, (rc, untouched)
        try:
            idx.pq_search_filtered(q, 10, prm, allowed=m50)
        except ValueError as ex:
            assert "LDS" in str(ex), str(ex)
        else:
            raise AssertionError("L = 577 was accepted although its state does not fit the LDS")
    check(H, ("envelope", ENVELOPE_L, "after the refusal"), q, 10, ENVELOPE_L, 64, [m50], "f16")
    check(H, ("envelope", 256), q, 10, 256, 64, [m50], "f16")
    H.close()
    print(f"LDS envelope: {fits} bytes accepted, {over} refused: ok", flush=True)


CASES["lds_envelope"] = case_lds_envelope


# ---- 8. rejections ---------------------------------------------------------------------------------------------------------------
def case_rejections(be):
    """Every LM_EINVAL / LM_ESTATE case of both entry points on sentinel-filled outputs that must keep their fill; n == 0; the empty index."""
    from leann_amd import _lib
    from leann_amd.index import Mi355xIndex

    lay = layout("m16-d64")
    x, g, q, cb, codes, off = pc._layout_inputs(lay, L2, be.emulated)
    q = np.ascontiguousarray(q[:2])
    words = pr.bitmap(draws(x.shape[0])[0])
    bare = Mi355xIndex.from_csr(g)  # no codes
    be.prepare(bare)
    H = Handle(be, g, cb, codes, off, x)  # codes, neither a provider nor a table
    idx = H.idx
    mk = idx.make_pq_params

    def both(tag, want, k, prm, index=idx, n=None, null=()):
        for device_form in (False, True):
            rc, _, _, untouched = raw(be, index, device_form, q, k, prm, words, n=n, null=null)
            assert rc == want and untouched, (tag, device_form, rc, untouched)

    rn = mk(16, 2)
    rn.recompute_neighbors = 1
    both("k 0", _lib.LM_EINVAL, 0, mk(16, 2))
    both("k -1", _lib.LM_EINVAL, -1, mk(16, 2))
    both("complexity 0", _lib.LM_EINVAL, 5, mk(0, 2))
    both("complexity -3", _lib.LM_EINVAL, 5, mk(-3, 2))
    both("recompute_neighbors", _lib.LM_EINVAL, 5, rn)
    both("beam_width 65", _lib.LM_EINVAL, 5, mk(16, 65))
    both("the LDS rule", _lib.LM_EINVAL, 5, mk(8000, 64, skip_search_reorder=True))
    both("NULL params", _lib.LM_EINVAL, 5, None)
    both("NULL index", _lib.LM_EINVAL, 5, mk(16, 2), null=("idx",))
    both("n < 0", _lib.LM_EINVAL, 5, mk(16, 2), n=-1)
    for name in ("x", "L", "D"):
        both("NULL " + name, _lib.LM_EINVAL, 5, mk(16, 2), null=(name,))
    both("no codes", _lib.LM_ESTATE, 5, mk(16, 2), index=bare)
    both("deferred fetch without a source", _lib.LM_ESTATE, 5, mk(16, 2, use_deferred_fetch=True))
    both("n == 0", 0, 5, mk(16, 2), n=0)
    for device_form in (False, True):  # the same call, accepted: the buffers are written
        rc, _, _, untouched = raw(be, idx, device_form, q, 5, mk(16, 2), words)
        assert rc == 0 and not untouched
    try:
        idx.pq_search_filtered(q, 5, mk(16, 65), allowed=[1, 2])
    except ValueError:
        pass
    else:
        raise AssertionError("must raise")
    bare.close()
    H.close()
    for metric, inf in ((L2, np.inf), (IP, -np.inf)):  # the empty index: every slot gets the empty values
        ge = pc.flat_csr([], 64, metric, -1)
        empty = open_index(be, ge, cb, np.zeros((0, 16), np.uint8), None)
        for device_form in (False, True):
            rc, lab, dist, _ = raw(be, empty, device_form, np.zeros((3, 64), np.float32), 4, mk(16, 2), None)
            assert rc == 0 and (lab == -1).all() and (dist == inf).all(), (metric, device_form)
        assert empty.get_option("filtered_allowed_evals") == 0
        empty.close()
    print("rejections: ok", flush=True)


CASES["rejections"] = case_rejections


# ---- 9. wrappers and backend wiring ----------------------------------------------------------------------------------------------
def case_wiring(be):
    """Mi355xIndex.pq_search_filtered / pq_search_filtered_device with ids, a bool mask and None; Mi355xDiskannSearcher.search(graph_filter=True,
    allowed_ids=...) on a bundle that keeps its vectors; the three ValueErrors."""
    import tempfile

    from leann_amd._compat import BACKEND_REGISTRY
    from leann_amd.backend import write_leann_bundle

    lay = layout("m16-d64")
    x, g, q, cb, codes, off = pc._layout_inputs(lay, L2, be.emulated)
    n = x.shape[0]
    q = np.ascontiguousarray(q[:4])
    k, L, W = 10, 40, 4
    mask = draws(n)[0]
    H = Handle(be, g, cb, codes, off, x)
    idx = H.idx
    idx.attach_table(x)
    prm = idx.make_pq_params(L, W)
    el, ed = H.R.expected(q, k, L, W, mask, x)[:2]
    ul, ud = H.R.expected(q, k, L, W, None, x)[:2]
    for allowed, (wl, wd) in ((np.flatnonzero(mask), (el, ed)), (mask, (el, ed)), (None, (ul, ud))):
        l, d = idx.pq_search_filtered(q, k, prm, allowed=allowed)
        assert d.shape == (4, k) and d.dtype == np.float32 and l.dtype == np.int64 and pr.same(l, d, wl, wd)
        if not be.emulated:
            import torch

            for a in (allowed, None if allowed is None else torch.from_numpy(pr.bitmap(mask).view(np.int32)).cuda()):
                ll, dd = idx.pq_search_filtered_device(torch.from_numpy(q).cuda(), k, prm, allowed=a)
                assert pr.same(ll.cpu().numpy(), dd.cpu().numpy(), wl, wd)
    assert pr.same(*idx.pq_search(q, k, prm), ul, ud)
    H.close()
    print("index wrappers: ok", flush=True)
    texts = [f"passage {i}" for i in range(n)]
    ids = [int(v) for v in np.flatnonzero(mask)]
    with tempfile.TemporaryDirectory() as td:
        p = str(Path(td) / "dk.leann")
        write_leann_bundle(p, texts, x, "sentence-transformers/all-MiniLM-L6-v2", backend_name="mi355x_diskann", distance_metric="l2")
        s = BACKEND_REGISTRY["mi355x_diskann"].searcher(p)
        be.prepare(s._ensure_index_loaded())
        # PQ order: the allowed entries of the plain search's final list are the best allowed nodes of E, so they head the filtered result.  (After an
        # exact rerank a node of F outside the final list may rank between them: only the count and the labels' membership are certain there.)
        kw = dict(complexity=20, beam_width=2, skip_search_reorder=True)
        plain = s.search(q, k, **kw)
        r = s.search(q, k, graph_filter=True, allowed_ids=ids, **kw)
        assert all(int(lab) in set(ids) for row in r["labels"] for lab in row if lab != "-1")
        kept = [[lab for lab in row if int(lab) in set(ids)] for row in plain["labels"]]
        assert all(sum(lab != "-1" for lab in row) >= len(kr) for row, kr in zip(r["labels"], kept))
        assert [row[: len(kr)] for row, kr in zip(r["labels"], kept)] == kept
        assert s.search(q, k, graph_filter=True, allowed_ids=mask, **kw)["labels"] == r["labels"]
        assert s.search(q, k, graph_filter=True, **kw)["labels"] == plain["labels"]
        rr = s.search(q, k, complexity=20, beam_width=2, graph_filter=True, allowed_ids=ids)  # reranked from the stored vectors
        assert all(int(lab) in set(ids) for row in rr["labels"] for lab in row if lab != "-1")
        assert [sum(lab != "-1" for lab in row) for row in rr["labels"]] == [sum(lab != "-1" for lab in row) for row in r["labels"]]
        for kw in (dict(allowed_ids=ids), dict(pq_flat=True, graph_filter=True, allowed_ids=ids), dict(pq_flat=True, graph_filter=True)):
            try:
                s.search(q, k, **kw)
            except ValueError:
                pass
            else:
                raise AssertionError(f"{kw} must raise ValueError")
        s.cleanup()
    print("searcher wiring: ok", flush=True)


CASES["wiring"] = case_wiring


def main(argv):
    import time

    import torch

    torch.set_num_threads(1)
    _load(argv[1])
    be = HostBackend()
    for name in argv[2:] or list(CASES):
        t0 = time.time()
        CASES[name](be)
        print(f"[case {name}: {time.time() - t0:.1f} s]", flush=True)
    print("ALL CASES OK", flush=True)


if __name__ == "__main__":
    main(sys.argv)
