"""Cases and reference for lm_graph_levels_to_csr_count / _fill and lm_graph_csr_to_level (csrc/lm_csr_impl.h), shared by the emulated CPU
run (tests/emulated_csr_cases.py) and the GPU run (tests/test_gpu_csr_kernel.py).  The reference is the project's own numpy assembly,
gpu_graph_build._assemble_csr (int64 arithmetic), followed by HnswCsr.validate()."""
import numpy as np

SCAN_TILE = 1024  # csrc/lm_csr_impl.h CSR_TILE: items per scan workgroup (256 lanes x 4)
NTOTALS = (0, 1, 1023, 1025, 2049 + 7)  # no tile, one node, a tile less one, two tiles, three tiles (the pointers: about twice as many)
CAPS = (4, 64, 96)  # the 16-lane group per row, its limit, the wave per row


def make_levels(ntotal: int, cap: int, seed: int = 0):
    """[(nodes int32 | None, adj int32 [n_rows, cap_l])]: level 0, upper levels of 37 and 3 nodes -- one of the 3 is not among the 37 --
    and a level without rows.  Rows in turn: with holes, all empty, full, with values outside [0, ntotal)."""
    rng = np.random.default_rng(seed + 1000 * cap + ntotal)
    n = ntotal

    def rows(nodes, c):  # the ids of a level's rows are nodes of that level, as the builder leaves them
        nr = nodes.shape[0]
        a = nodes[rng.integers(0, max(nr, 1), (nr, c))].astype(np.int32).reshape(nr, c)
        kind = (np.arange(nr) % 4)[:, None]
        a[(rng.random((nr, c)) < 0.4) & (kind == 0)] = -1
        a[np.broadcast_to(kind == 1, a.shape)] = -1
        out = (rng.random((nr, c)) < 0.3) & (kind == 3)
        a[out] = rng.choice(np.array([-7, n, n + 5, 2**31 - 1, -(2**31)]), int(out.sum())).astype(np.int32)
        return a

    nodes1 = np.sort(rng.choice(n, min(37, max(n - 1, 0)), replace=False)).astype(np.int32)
    outside = np.setdiff1d(np.arange(n, dtype=np.int32), nodes1)
    nodes2 = np.sort(np.concatenate([rng.choice(outside, min(1, n), replace=False), rng.choice(nodes1, min(2, nodes1.shape[0]), replace=False)])).astype(np.int32)
    none = np.zeros(0, np.int32)
    return [(None, rows(np.arange(n, dtype=np.int32), cap)), (nodes1, rows(nodes1, max(cap // 2, 1))), (nodes2, rows(nodes2, cap)), (none, rows(none, cap))]


def reference(levels, ntotal: int):
    from leann_amd.gpu_graph_build import _assemble_csr

    top = np.zeros(ntotal, np.int64)
    graphs = []
    for l, (nodes, adj) in enumerate(levels):
        sub = np.arange(ntotal, dtype=np.int64) if nodes is None else nodes.astype(np.int64)
        top[sub] = l
        a = adj.astype(np.int64)
        ok = (a >= 0) & (a < ntotal)
        a[ok] = np.searchsorted(sub, a[ok])  # _assemble_csr takes ids local to the level's node list
        a[~ok] = -1  # the contract's empty slot, in the form _assemble_csr knows
        graphs.append((sub, a))
    g = _assemble_csr(top, graphs, np.arange(ntotal, dtype=np.int64), 8, 0, int(np.argmax(top)) if ntotal else -1, 2, 10)
    g.validate()
    return g


def reference_level(g, level: int, nodes, cap: int):
    ids = np.arange(g.ntotal) if nodes is None else nodes
    adj, deg, over = np.full((len(ids), cap), -1, np.int32), np.zeros(len(ids), np.int32), 0
    for r, v in enumerate(ids):
        if g.levels[v] > level:
            lst = g.neighbors_of(int(v), level)
            deg[r] = min(len(lst), cap)
            adj[r, : deg[r]] = lst[: deg[r]]
            over += len(lst) - deg[r]
    return adj, deg, over


def check_case(dev, ntotal: int, cap: int):
    """Both directions on ``dev`` ("cpu": the emulated library), byte for byte against the reference."""
    import torch

    from leann_amd import gpu_graph_build as gb

    levels = make_levels(ntotal, cap)
    ref = reference(levels, ntotal)
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    got = [x.cpu().numpy() for x in gb.levels_to_csr_kernel([(t(nd), t(a)) for nd, a in levels], ntotal)]
    for name, a, e in zip(("levels", "node_offsets", "level_ptr", "neighbors"), got, (ref.levels, ref.node_offsets, ref.level_ptr, ref.neighbors)):
        assert a.tobytes() == e.tobytes(), (name, ntotal, cap)
    csr = (t(ref.levels), t(ref.node_offsets.view(np.int64)), t(ref.level_ptr.view(np.int64)), t(ref.neighbors))
    # level 0 as it is; at half the cap (the full rows overflow); the upper levels by their own nodes; a level above every node's top
    for level, nodes, c in ((0, None, cap), (0, None, max(cap // 2, 1)), (1, levels[1][0], cap), (2, levels[2][0], 3), (len(levels), None, cap)):
        adj, deg, over = gb.level_from_csr_kernel(*csr, level, c, t(nodes))
        e_adj, e_deg, e_over = reference_level(ref, level, nodes, c)
        assert adj.cpu().numpy().tobytes() == e_adj.tobytes() and deg.cpu().numpy().tobytes() == e_deg.tobytes() and int(over) == e_over, (level, c, ntotal, cap)
    if ntotal > 4:
        assert reference_level(ref, 0, None, max(cap // 2, 1))[2] > 0  # the case does overflow
