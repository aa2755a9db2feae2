"""Helpers shared by the view-index tests (tests/test_graph_view.py on the CPU, tests/test_gpu_graph_view.py on the MI355X): the CSR graph
that lm_index_create_view's contract declares a list of levels equivalent to, the oracle's form of it, and layered test graphs in
lm_graph_add_links' fixed-capacity layout (holes, a full row, an empty row, a top level of one node).

A level is a pair (nodes, adj): ``nodes`` an ascending int32 array of the node ids the level lists (None = identity: row r is node r),
``adj`` an int32 array [n_rows, cap] whose values outside [0, ntotal) are empty slots."""
from __future__ import annotations

import numpy as np


def compose_csr(levels, ntotal: int, d: int, metric: int, entry_point: int, carry=None):
    """The equivalent CSR of include/leann_mi355x.h ("Equivalence"): node v carries levels 0 .. top(v), top(v) = the highest level that
    lists v; each list = the non-empty slots of v's row in slot order, empty where a level at or below top(v) does not list v.
    ``carry`` {v: level}: v carries (empty) lists up to that level although no level lists it there -- what a CSR needs to express "a link at
    that level names v" (a CSR walk that arrives at v reads v's list of that level; the view finds no row and reads nothing)."""
    from leann_amd.csr_format import csr_from_adjacency

    top = np.zeros(ntotal, np.int64)
    rows = []
    for l, (nodes, adj) in enumerate(levels):
        ids = np.arange(adj.shape[0], dtype=np.int64) if nodes is None else np.asarray(nodes, np.int64)
        assert np.all(ids[1:] > ids[:-1]) and (ids.size == 0 or (ids[0] >= 0 and ids[-1] < ntotal))
        top[ids] = l
        rows.append({int(v): r for r, v in enumerate(ids)})
    for v, l in (carry or {}).items():
        top[v] = max(top[v], l)
    per_node = []
    for v in range(ntotal):
        lists = []
        for l in range(int(top[v]) + 1):
            r = rows[l].get(v)
            if r is None:
                lists.append(np.zeros(0, np.int32))
            else:
                a = np.asarray(levels[l][1][r], np.int64)
                lists.append(a[(a >= 0) & (a < ntotal)].astype(np.int32))
        per_node.append(lists)
    g = csr_from_adjacency(per_node, d, metric, entry_point if ntotal else -1)
    g.validate()
    return g


def oracle_of(levels, ntotal: int, d: int, metric: int, entry_point: int, carry=None):
    """(the composed CSR, the oracle's graph over it)."""
    from tests.util import oracle_graph

    g = compose_csr(levels, ntotal, d, metric, entry_point, carry)
    return g, oracle_graph(g, d)


def levels_from_csr(g, caps, rng, single_top: bool = True):
    """Thin a built HNSW graph into fixed-capacity levels: level l keeps the first caps[min(l, len(caps) - 1)] links of every list, scattered
    over the row's slots in order with -1 holes between them (and one out-of-range value standing for an empty slot, as the header allows);
    per level one row filled to cap and one emptied; with ``single_top`` a further top level that lists the entry point alone.
    Every upper-level link names a node of that level.  Returns (levels, entry_point)."""
    n = g.ntotal
    levels = []
    for l in range(g.max_level + 1):
        cap = caps[min(l, len(caps) - 1)]
        ids = np.nonzero(g.levels > l)[0].astype(np.int32)
        adj = np.full((ids.shape[0], cap), -1, np.int32)
        for r, v in enumerate(ids):
            nb = g.neighbors_of(int(v), l)[:cap]
            adj[r, np.sort(rng.permutation(cap)[: nb.shape[0]])] = nb
        if ids.shape[0] >= 3:
            full, empty = rng.permutation(ids.shape[0])[:2]
            if ids[full] == g.entry_point or ids[empty] == g.entry_point:
                full, empty = [r for r in range(ids.shape[0]) if ids[r] != g.entry_point][:2]
            others = ids[ids != ids[full]]
            adj[full] = others[rng.permutation(others.shape[0])[:cap]] if others.shape[0] >= cap else adj[full]
            adj[empty] = -1
            holes = np.argwhere(adj == -1)
            if holes.shape[0]:  # an empty slot need not be -1: anything outside [0, ntotal) is one
                adj[tuple(holes[rng.integers(0, holes.shape[0])])] = n + 7
        levels.append((None if l == 0 else ids, adj))
    if single_top:
        levels.append((np.array([g.entry_point], np.int32), np.full((1, caps[-1]), -1, np.int32)))
    return levels, int(g.entry_point)


def as_tensors(levels, device=None):
    """The levels as Mi355xIndex.from_levels takes them (int32 tensors, on ``device`` when given)."""
    import torch

    out = []
    for nodes, adj in levels:
        a = torch.from_numpy(np.ascontiguousarray(adj, np.int32))
        nd = None if nodes is None else torch.from_numpy(np.ascontiguousarray(nodes, np.int32))
        if device is not None:
            a, nd = a.to(device), (None if nd is None else nd.to(device))
        out.append((nd, a))
    return out


def same_result(got, exp) -> bool:
    """(distances, labels) pairs: labels equal, distances equal as bit patterns."""
    return np.array_equal(np.asarray(got[1]), np.asarray(exp[1])) and np.asarray(got[0], np.float32).tobytes() == np.asarray(exp[0], np.float32).tobytes()
