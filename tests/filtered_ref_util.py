"""The reference of lm_index_search_filtered, COMPOSED from the unmodified oracle (oracle.search, oracle.bruteforce_topk, oracle.dist) -- the search
is not restated.  For one query:
    1. the seed: oracle.search on a copy of the graph whose level-0 lists are all empty.  The upper-level descent is the full graph's, the
       pool then holds only the node it hands to level 0: label 0 is the seed;
    2. E: oracle.search for that query on a level-0-only copy (max_level 0, entry point = seed) with a recording provider that serves rows of
       the test's table.  A one-query search asks the provider for exactly its new-lists (the first one is the entry point itself), so the
       union of the request lists is E, seed included;
    3. the composition is checked: labels and distance bits of that run equal those of the oracle on the FULL graph;
    4. expected = the first k of E n allowed under the oracle's key: oracle.bruteforce_topk over the served rows of E n allowed (ids ascending,
       so the lower-id tie-break carries over; a sample of its distances is compared with oracle.dist of the same rows).
E depends on everything that steers the walk (k included: the pool holds max(ef, k) keys), never on the allow-list."""
from __future__ import annotations

import numpy as np

from tests.gpu_exact_util import bitmap, expected as _topk, pad64, same  # noqa: F401  (re-exported for the case list)

IP, L2 = 0, 1


def _lists(g):
    """per node: [level-0 list, level-1 list, ...] of the compact CSR"""
    out = []
    for i in range(g.ntotal):
        p0, p1 = int(g.node_offsets[i]), int(g.node_offsets[i + 1])
        out.append([g.neighbors[int(g.level_ptr[p]) : int(g.level_ptr[p + 1])] for p in range(p0, p1 - 1)])
    return out


def _csr(g, lists, entry_point, max_level):
    from leann_amd.csr_format import HnswCsr

    levels = np.array([len(ls) for ls in lists], np.int32)
    node_offsets = np.concatenate([[0], np.cumsum(levels.astype(np.int64) + 1)]).astype(np.uint64)
    level_ptr = np.zeros(int(node_offsets[-1]), np.uint64)
    nb, pos = [], 0
    for i, ls in enumerate(lists):
        p = int(node_offsets[i])
        for lst in ls:
            level_ptr[p] = pos
            pos += len(lst)
            nb.append(np.asarray(lst, np.int32))
            p += 1
        level_ptr[p] = pos
    neighbors = np.concatenate(nb + [np.zeros(0, np.int32)]).astype(np.int32)
    return HnswCsr(d=g.d, ntotal=g.ntotal, metric_type=g.metric_type, levels=levels, level_ptr=level_ptr, node_offsets=node_offsets,
                   neighbors=neighbors, entry_point=entry_point, max_level=max_level)


def without_level0(g):
    """the same graph with every level-0 list empty"""
    return _csr(g, [[ls[0][:0]] + list(ls[1:]) for ls in _lists(g)], g.entry_point, g.max_level)


def level0_only(g, seed: int):
    """level 0 alone, entered at `seed`"""
    return _csr(g, [[ls[0]] for ls in _lists(g)], int(seed), 0)


class Reference:
    """One graph + the table its rows are served from (fp32 values: an fp16 table widened)."""

    def __init__(self, g, table: np.ndarray):
        from tests.util import oracle_graph

        self.g, self.table = g, np.ascontiguousarray(table, np.float32)
        self.metric, self.d = int(g.metric_type), int(g.d)
        self.full = oracle_graph(g, self.d)
        self.upper = oracle_graph(without_level0(g), self.d)
        self._l0 = _lists(g)
        self._seed, self._E, self._og0 = {}, {}, {}

    def seed(self, q1: np.ndarray) -> int:
        from oracle import oracle as orc

        key = q1.tobytes()
        if key not in self._seed:
            ids, _, _ = orc.search(self.upper, q1[None], 1, ef=1, table=self.table)
            self._seed[key] = int(ids[0, 0])
        return self._seed[key]

    def evaluated(self, q1: np.ndarray, k: int, ef: int, beam: int = 1, batch_size: int = 0, check: bool = True) -> np.ndarray:
        """E of one query: sorted unique ids (steps 1-3)"""
        from oracle import oracle as orc
        from tests.util import oracle_graph

        key = (q1.tobytes(), k, ef, beam, batch_size, check)
        if key in self._E:
            return self._E[key]
        s = self.seed(q1)
        if s not in self._og0:
            self._og0[s] = oracle_graph(_csr(self.g, [[ls[0]] for ls in self._l0], s, 0), self.d)
        asked = []
        li, ld, _ = orc.search(self._og0[s], q1[None], k, ef=ef, beam=beam, check_relative_distance=check, batch_size=batch_size,
                               provider=lambda idv: (asked.append(idv.copy()), self.table[idv])[1])
        fi, fd, _ = orc.search(self.full, q1[None], k, ef=ef, beam=beam, check_relative_distance=check, batch_size=batch_size, table=self.table)
        assert same(li, ld, fi, fd), "the composition (seed + level-0-only walk) is not the oracle's search on the full graph"
        E = np.unique(np.concatenate(asked))
        assert sum(a.size for a in asked) == E.size and s in E  # a one-query walk meets every node once
        self._E[key] = E
        return E

    def expected(self, q: np.ndarray, k: int, mask: np.ndarray | None, ef: int, beam: int = 1, batch_size: int = 0, check: bool = True):
        """(labels [nq, k], distances [nq, k], sum over the queries of |E n allowed|, hits per query)"""
        from oracle import oracle as orc

        labs, dists, evals, hits = [], [], 0, []
        tab, qp = pad64(self.table), pad64(np.ascontiguousarray(q, np.float32))
        for i in range(q.shape[0]):
            E = self.evaluated(np.ascontiguousarray(q[i], np.float32), k, ef, beam, batch_size, check)
            sel = np.zeros(self.g.ntotal, bool)
            sel[E] = True
            if mask is not None:
                sel &= mask
            lab, dd = _topk(tab, qp[i : i + 1], k, self.metric, sel)
            for j in range(min(3, int((lab[0] >= 0).sum()))):  # bruteforce_topk's distances ARE oracle.dist of the served rows
                dj = np.float32(orc.dist(self.table[lab[0, j]], q[i], self.metric))
                want = dd[0, j] if self.metric == L2 else -dd[0, j]
                assert (np.isnan(dj) and np.isinf(want)) or dj == want, (dj, want)
            labs.append(lab[0])
            dists.append(dd[0])
            evals += int(sel.sum())
            hits.append(int(min(k, sel.sum())))
        return np.stack(labs), np.stack(dists), evals, np.array(hits)
