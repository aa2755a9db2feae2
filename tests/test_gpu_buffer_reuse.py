"""The host-pointer entry points on ONE index on the MI355X: they share the index's grow-only device buffers (csrc/lm_devbuf.h: query / result
staging, the padded queries, the uploaded allow-list, the per-query counters, the workspaces).  The sequence of
tests/hip_emul/run_buffer_reuse.cpp -- N = 400, D = 48 (padded to 64), PQ with m = 4; k = 3, then 10; n = 1, 5, 2, 9; every entry point in turn,
the allow-list going round None, every node, every third node -- and every result bit-equal to the same call on a fresh index."""
import numpy as np
import pytest


def _has_gpu() -> bool:
    try:
        import torch

        return torch.cuda.is_available()
    except Exception:  # noqa: BLE001
        return False


pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not _has_gpu(), reason="needs an MI355X")]

N, D, DP, M = 400, 48, 64, 4


def _world():
    from leann_amd.csr_format import HnswCsr

    rng = np.random.default_rng(12345)
    i = np.arange(N, dtype=np.float32)[:, None]
    j = np.arange(D, dtype=np.float32)[None, :]
    table = (np.cos(6.2831853 * i / N + 0.37 * j) + 0.3 * (rng.random((N, D)) - 0.5)).astype(np.float32)
    levels = np.where(np.arange(N) % 16 == 0, 2, 1).astype(np.int32)
    level_ptr, neighbors = [], []
    for v in range(N):  # the two-level ring with chords of tests/hip_emul/run_filtered_search.cpp
        level_ptr.append(len(neighbors))
        neighbors += [(v + d) % N for d in (1, N - 1, 2, N - 2, 7, 31, N - 45)]
        if levels[v] == 2:
            level_ptr.append(len(neighbors))
            neighbors += [(v + d) % N for d in (16, N - 16, 64)]
        level_ptr.append(len(neighbors))
    node_offsets = np.concatenate([[0], np.cumsum(levels + 1)]).astype(np.uint64)
    g = HnswCsr(d=D, ntotal=N, metric_type=1, levels=levels, level_ptr=np.asarray(level_ptr, np.uint64), node_offsets=node_offsets,
                neighbors=np.asarray(neighbors, np.int32), entry_point=0, max_level=1)
    dsub = D // M
    codebooks = np.stack([table[(np.arange(256) * 25 + c) % N, c * dsub:(c + 1) * dsub] for c in range(M)])  # (m, 256, d/m): rows of the table
    codes = np.stack([((table[:, None, c * dsub:(c + 1) * dsub] - codebooks[c][None]) ** 2).sum(-1).argmin(1) for c in range(M)], axis=1).astype(np.uint8)
    q = (table[(37 + 71 * np.arange(9)) % N] + 0.05 * (rng.random((9, D)) - 0.5)).astype(np.float32)
    return g, table, codebooks, codes, q


def test_every_host_pointer_entry_point_in_turn_on_one_index_equals_a_fresh_index():
    import torch

    from leann_amd import _lib
    from leann_amd.devmem import as_tensor
    from leann_amd.index import Mi355xIndex

    _lib.require_gpu()
    g, table, codebooks, codes, q = _world()
    assert g.metric_type == _lib.METRIC_L2
    padded = torch.zeros((N, DP), dtype=torch.float32, device="cuda")
    padded[:, :D] = torch.from_numpy(table).cuda()
    keep = {}

    def provider(d_ids, cnt, stream):
        keep["e"] = padded.index_select(0, as_tensor(d_ids, (cnt,), "int32").long()).contiguous()
        return keep["e"].data_ptr()

    def make_index():
        idx = Mi355xIndex.from_csr(g, device=0)
        idx.set_stream(torch.cuda.current_stream().cuda_stream)
        idx.attach_table(table)
        idx.set_provider(provider)
        idx.attach_pq(codebooks, codes)
        return idx

    sp = lambda **kw: Mi355xIndex.make_params(ef=16, **kw)  # noqa: E731
    pp = Mi355xIndex.make_pq_params(complexity=24)

    def profiled(ix, x, k, a):
        ix.set_profiling(True)
        try:
            return ix.search(x, k, sp())
        finally:
            ix.set_profiling(False)

    # (distances, labels) of one call; lm_index_search's five forms first, then the five other entry points
    ops = [
        ("search stored", lambda ix, x, k, a: ix.search(x, k, sp(recompute=False))),
        ("search recompute", lambda ix, x, k, a: ix.search(x, k, sp())),
        ("search stored pruned", lambda ix, x, k, a: ix.search(x, k, sp(recompute=False, prune_ratio=0.5))),
        ("search recompute pruned", lambda ix, x, k, a: ix.search(x, k, sp(prune_ratio=0.5))),
        ("search profiled", profiled),
        ("search_filtered", lambda ix, x, k, a: ix.search_filtered(x, k, sp(recompute=bool(len(x) % 2)), a)),
        ("search_exact", lambda ix, x, k, a: ix.search_exact(x, k, a)),
        ("pq_search", lambda ix, x, k, a: ix.pq_search(x, k, pp)[::-1]),
        ("pq_search_filtered", lambda ix, x, k, a: ix.pq_search_filtered(x, k, pp, a)[::-1]),
        ("pq_flat_search", lambda ix, x, k, a: ix.pq_flat_search(x, k, pp, a)[::-1]),
    ]
    allows = [None, np.ones(N, dtype=bool), np.arange(N) % 3 == 0]
    shared = make_index()
    turn = 0
    for k in (3, 10):
        for n in (1, 5, 2, 9):
            for i in range(10):
                name, fn = ops[(i % 2) * 5 + (i // 2 + turn) % 5]  # the two halves alternate; where each starts moves with every turn
                allow = allows[(turn + i) % 3]
                d_s, l_s = fn(shared, q[:n], k, allow)
                fresh = make_index()
                d_f, l_f = fn(fresh, q[:n], k, allow)
                fresh.close()
                what = f"{name}, n = {n}, k = {k}, allow-list {(turn + i) % 3}"
                assert l_s.shape == (n, k) and (l_s >= 0).any(), what
                assert np.array_equal(l_s, l_f), what
                assert np.array_equal(d_s.view(np.uint32), d_f.view(np.uint32)), what
            turn += 1
    shared.close()
