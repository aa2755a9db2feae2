"""The reference of lm_pq_batch_search_filtered, COMPOSED from the unmodified oracle (oracle.pq_lut_adc, oracle.pq_search,
oracle.bruteforce_topk).  For one query:
    1. every ADC distance comes from oracle.pq_lut_adc (orc_pq_lut + orc_pq_adc);
    2. a short restatement of orc_pq_search's walk runs over those values -- visited set, the W closest unexpanded entries of the list of
       L = max(L, k) keys, a hop evaluated as a set and then merged, stop when nothing is left to expand -- and RECORDS E, the evaluated
       nodes, hop by hop;
    3. the composition is checked on every query: the walk's final list (labels and PQ-order distance bits, skip_search_reorder) and its
       n_adc / n_expand / n_rounds equal oracle.pq_search's for that query;
    4. F = the first L of E n allowed under the key (adc, id): NaN ranks as +inf, -0 as +0, ties go to the lower id;
    5. expected = F in PQ order (inner product decoded as the negation), or oracle.bruteforce_topk over the rows of F with ids ascending
       (as tests/filtered_ref_util.py) for the table, fp16 and deferred modes; the expected provider request is the sorted unique union
       of the F lists of a pass.
E depends on everything that steers the walk (k included: the list holds max(L, k) keys), never on the allow-list."""
from __future__ import annotations

import numpy as np

from tests.gpu_exact_util import bitmap, expected as _topk, pad64, same  # noqa: F401  (re-exported for the case list)
from tests.pq_flat_ref_util import rank

IP, L2 = 0, 1
FS = 64             # csrc/lm_pq_impl.h: PQ_FILTER_STAGE
LDS_LIMIT = 158 * 1024


def next_pow2(v):
    p = 1
    while p < v:
        p <<= 1
    return p


def lds_bytes_filtered(max_degree0: int, m: int, L: int, W: int) -> int:
    """the header's LDS rule: the unfiltered bytes + 8 L + 8 FS"""
    new = max(W * max_degree0, 1)
    return m * 1024 + 24 * L + 8 * next_pow2(new) + 4 * new + 8 * FS


def _canon(d):
    with np.errstate(invalid="ignore"):
        d = np.where(np.isnan(d), np.float32(np.inf), d).astype(np.float32)
    return np.where(d == 0, np.float32(0.0), d).astype(np.float32)


def _order(ids, adc):
    """indices that sort (adc, id) ascending under the key"""
    return np.lexsort((ids, _canon(adc)))


class Reference:
    """One single-level graph + quantiser; `x` are the rows a rerank is served from (fp32 values: an fp16 table widened)."""

    def __init__(self, g, cb, codes, off=None):
        from tests.util import oracle_graph

        self.g, self.cb, self.codes, self.off = g, cb, codes, off
        self.n, self.d, self.metric = int(g.ntotal), int(g.d), int(g.metric_type)
        self.og = oracle_graph(g, self.d)
        lp = g.level_ptr
        no = g.node_offsets
        self.adj = [g.neighbors[int(lp[int(no[i])]) : int(lp[int(no[i]) + 1])] for i in range(self.n)]
        self._adc, self._walk = {}, {}

    def adc_all(self, q1):
        """orc_pq_adc of every node for one query (from oracle.pq_lut_adc)"""
        from oracle import oracle as orc

        key = q1.tobytes()
        if key not in self._adc:
            _, a = orc.pq_lut_adc(self.cb, self.codes, np.ascontiguousarray(q1, np.float32), self.metric, np.arange(self.n), chunk_off=self.off)
            self._adc[key] = a
        return self._adc[key]

    def walk(self, q1, k, L, W):
        """-> dict(E: evaluated ids in hop order, hops: the fresh ids of every hop (hop 0 = the entry point), lst: the final list's ids in key
        order, n_adc, n_expand, n_rounds); checked against oracle.pq_search (step 3)"""
        from oracle import oracle as orc

        L = max(L, k)
        key = (q1.tobytes(), L, W)
        if key in self._walk:
            return self._walk[key]
        adc = self.adc_all(q1)
        ep = int(self.g.entry_point)
        vis = np.zeros(self.n, bool)
        vis[ep] = True
        ids, exp = np.array([ep], np.int64), np.array([False])
        hops, nexp, rounds = [np.array([ep], np.int64)], 0, 0
        while True:
            un = np.flatnonzero(~exp)[:W]  # ids is kept in key order
            if un.size == 0:
                break
            rounds += 1
            nexp += un.size
            exp[un] = True
            fresh = []
            for p in ids[un]:
                for v in self.adj[int(p)].tolist():
                    if not vis[v]:
                        vis[v] = True
                        fresh.append(v)
            fresh = np.array(fresh, np.int64)
            hops.append(fresh)
            ids = np.concatenate([ids, fresh])
            exp = np.concatenate([exp, np.zeros(fresh.size, bool)])
            o = _order(ids, adc[ids])[:L]
            ids, exp = ids[o], exp[o]
        E = np.concatenate(hops)
        w = dict(E=E, hops=hops, lst=ids, n_adc=int(E.size), n_expand=nexp, n_rounds=rounds + 1)
        oi, od, ost = orc.pq_search(self.og, self.cb, self.codes, q1[None], L, L=L, W=W, skip_search_reorder=True, chunk_off=self.off)
        li, ld = rank(adc[ids], ids, L, self.metric)
        assert same(li[None], ld[None], oi, od), "the restated walk's final list is not oracle.pq_search's"
        assert (w["n_adc"], w["n_expand"], w["n_rounds"]) == (ost["n_adc"], ost["n_expand"], ost["n_rounds"]), (w, ost)
        self._walk[key] = w
        return w

    def flist(self, q1, k, L, W, mask):
        """F: ids in key order, and |E n allowed|"""
        E = self.walk(q1, k, L, W)["E"]
        A = E if mask is None else E[mask[E]]
        adc = self.adc_all(q1)
        return A[_order(A, adc[A])[: max(L, k)]], int(A.size)

    def expected(self, q, k, L, W, mask, table=None):
        """table None: the PQ order; else the exact rerank over its rows (fp32 values).
        -> (labels [nq, k], distances [nq, k], sum |E n allowed|, hits per query, sorted unique union of the F lists, (ndis, nexpand, nrounds))"""
        labs, dists, evals, hits, union = [], [], 0, [], []
        st = [0, 0, 0]
        qp = pad64(np.ascontiguousarray(q, np.float32))
        tab = None if table is None else pad64(np.ascontiguousarray(table, np.float32))
        for i in range(q.shape[0]):
            q1 = np.ascontiguousarray(q[i], np.float32)
            w = self.walk(q1, k, L, W)
            F, na = self.flist(q1, k, L, W, mask)
            if tab is None:
                lab, dd = rank(self.adc_all(q1)[F], F, max(max(L, k), 1), self.metric)
                lab, dd = lab[:k], dd[:k]
            else:
                sel = np.zeros(self.n, bool)
                sel[F] = True
                lab, dd = _topk(tab, qp[i : i + 1], k, self.metric, sel)
                lab, dd = lab[0], dd[0]
            labs.append(lab)
            dists.append(dd)
            evals += na
            hits.append(min(k, F.size))
            union.append(F)
            st = [st[0] + w["n_adc"], st[1] + w["n_expand"], max(st[2], w["n_rounds"])]
        un = np.unique(np.concatenate(union)).astype(np.int32) if union else np.zeros(0, np.int32)
        return np.stack(labs), np.stack(dists), evals, np.array(hits), un, tuple(st)

    def post_filter_hits(self, q1, k, L, W, mask):
        """what the reference's post-filter keeps of the final list (ids in list order)"""
        lst = self.walk(q1, k, L, W)["lst"]
        return lst[mask[lst]]
