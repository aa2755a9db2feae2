"""The wide padded widths (1536 .. 4096: csrc/lm_wide_impl.h) against the oracle: labels, distance bits and stats equal.  Worlds, graphs and
comparisons are tests/emulated_graph_search_cases.py's and tests/gpu_exact_util.py's; the shapes live here.  tests/test_gpu_wide_widths.py
runs them on the MI355X, tests/test_wide_widths.py on the host build of the library at 1536 and 4096:
    python -m tests.emulated_wide_cases <path/to/libleann_mi355x_emul.so> [case ...]"""
import ctypes as C
import sys

import numpy as np

from tests.emulated_graph_search_cases import IP, L2, LOCKSTEP_LDS, PERSIST_LDS, HostBackend, Scenario, _load, assert_refused, layered_graph, next_pow2, raw_search

WIDTHS = (1536, 2048, 2560, 3072, 4096)
TABLE_WORLDS = ("persist_wg", "persist_wave", "lock_wg", "lock_wave")  # (the wave options are served by the 256-thread kernels)


def scenario(dp, metric, d, beam, n, batch_size=0, ef=32):
    """A layered graph of n nodes (degrees 3 .. 12, three levels), 9 queries, k = 10.  Beam 4 x degree 12 gives new-lists of more than 32 rows:
    more than one pass of 16 groups x 2 rows, odd tails included."""
    rng = np.random.default_rng(dp + 7 * metric + d % 5 + beam)
    x = (1.5 * rng.standard_normal((n, d))).astype(np.float32)
    q = (x[rng.integers(0, n, 9)] + 0.4 * rng.standard_normal((9, d))).astype(np.float32)
    return Scenario(("wide", dp, d, metric, beam, batch_size, ef), layered_graph(n, d, metric, 3000 + dp), x, q, 10, ef, beam=beam, batch_size=batch_size)


def run_search(be, dp, metric, n, ds=None, f16s=(False, True), worlds=TABLE_WORLDS, beams=(1, 4)):
    """The stored table: zero padding and none, beam 1 and 4; and the lock-step rounds with dynamic batching."""
    for d in ds or (dp - 3, dp):
        for beam in beams:
            scenario(dp, metric, d, beam, n).run(be, worlds=worlds, f16s=f16s)
    scenario(dp, metric, dp - 3, 1, n, batch_size=8).run(be, worlds=("lock_wg",), f16s=f16s[:1])


def run_provider(be, dp, metric, n, worlds=("rank_wg", "rank_wave", "identity", "memo")):
    """recompute = 1: rank addressing, identity, memo slot; results, stats and every round's request list are the oracle's."""
    scenario(dp, metric, dp - 3, 4, n).run(be, worlds=worlds)


def gather_case(dp, f16, npairs, metric):
    """(table, queries, qidx, ids, orc_dist of the pairs): 37 rows -- row 5 holds a NaN, row 6 is all zero --, 3 queries."""
    from oracle import oracle as orc

    rng = np.random.default_rng(dp + npairs)
    tab = rng.standard_normal((37, dp)).astype(np.float32)
    tab[5, dp - 1], tab[6] = np.nan, 0.0
    tab = tab.astype(np.float16) if f16 else tab
    q, qidx, ids = rng.standard_normal((3, dp)).astype(np.float32), rng.integers(0, 3, npairs).astype(np.int32), rng.integers(0, 37, npairs).astype(np.int32)
    ids[: min(npairs, 2)] = (5, 6)[: min(npairs, 2)]
    return tab, q, qidx, ids, np.array([orc.dist(tab[i].astype(np.float32), q[j], metric) for j, i in zip(qidx, ids)], np.float32)


def exact_case(dp, ntable, nq, f16, metric, masked):
    """gauss_case's table (its second half a copy of the first) and a random half as the allow-list -> (table, q, words, expected labels, distances)"""
    from tests import gpu_exact_util as xu

    table, q = xu.gauss_case(ntable, dp, nq, dp + ntable + nq, f16)
    mask = np.random.default_rng(dp).random(ntable) < 0.5 if masked else None
    return (table, q, None if mask is None else xu.bitmap(mask)) + tuple(xu.expected(table, q, 10, metric, mask))


def run_envelope(be, n):
    """4096 wide, the header's LDS rules from both sides: ef_p / ef_l = the largest efSearch of the persistent launch / the lock-step rounds."""
    from leann_amd.index import Mi355xIndex

    sc = scenario(4096, L2, 4096, 1, n)
    idx = Mi355xIndex.from_csr(sc.g)
    be.prepare(idx)
    maxnew = max(int(idx.info.max_degree0), int(idx.info.max_degree_up), 1)
    fixed = max(next_pow2(maxnew), 2) * 8 + 4 * 4096
    ef_p, ef_l = (PERSIST_LDS - fixed - 4 * maxnew) // 16, (LOCKSTEP_LDS - fixed) // 16
    assert 10 < ef_l < ef_p
    scenario(4096, L2, 4096, 1, n, ef=ef_p).run(be, worlds=("persist_wg",), idx=idx)
    assert_refused(("wide", ef_p + 1), idx, sc.q, 10, idx.make_params(ef=ef_p + 1, recompute=False))
    scenario(4096, L2, 4096, 1, n, ef=ef_l).run(be, worlds=("lock_wg",), idx=idx)
    idx.set_option("persistent_table", 0)
    assert_refused(("wide lock-step", ef_l + 1), idx, sc.q, 10, idx.make_params(ef=ef_l + 1, recompute=False))
    scenario(4096, L2, 4096, 1, n, ef=ef_l + 1).run(be, worlds=("persist_wg",), idx=idx)  # what the lock-step rounds refuse, the persistent launch serves
    idx.close()


def run_refusals(be):
    """Width 1088 stays refused; at 1536 every entry point without a wide form returns LM_EINVAL and leaves its outputs alone (the build-time
    entry points check the width before they look at a buffer: host arrays serve on the GPU too)."""
    from leann_amd import _lib
    from leann_amd.index import Mi355xIndex

    def refused(rc, *outs):
        assert rc == _lib.LM_EINVAL and "unsupported padded dimension" in _lib.last_error(), (rc, _lib.last_error())
        assert all(np.all(o == o.flat[0]) and o.flat[0] in (123.25, -77) for o in outs), "a refused call wrote to its outputs"

    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for d, dp in ((1025, 1088), (1533, 1536)):
        sc = scenario(dp, L2, d, 1, 40)
        idx = Mi355xIndex.from_csr(sc.g)
        be.prepare(idx)
        assert int(idx.info.d_padded) == dp
        idx.attach_table(sc.x)
        prm = idx.make_params(ef=32, recompute=False)
        if dp == 1088:
            refused(*raw_search(idx, sc.q, 10, prm)[:3])
            idx.close()
    lib, q, n = idx._lib, sc.q, sc.q.shape[0]
    dist, labels = np.full((n, 10), 123.25, np.float32), np.full((n, 10), -77, np.int64)
    refused(lib.lm_index_search_filtered(idx._h, n, ptr(q), 10, None, ptr(dist), ptr(labels), C.byref(prm)), dist, labels)
    prm.pq_pruning_ratio = 0.5
    refused(*raw_search(idx, q, 10, prm)[:3])
    cb, codes, off = np.zeros((4, 256, 384), np.float32), np.zeros((40, 4), np.uint8), np.array([0, 384, 768, 1152, 1533], np.int32)
    refused(lib.lm_pq_attach_chunked(idx._h, 4, ptr(off), ptr(cb), ptr(codes), 40))
    pp = _lib.PqSearchParams()
    lib.lm_pq_search_params_default(C.byref(pp))
    refused(lib.lm_pq_batch_search(idx._h, n, ptr(q), 10, C.byref(pp), ptr(labels), ptr(dist)), dist, labels)
    refused(lib.lm_pq_batch_search_filtered(idx._h, n, ptr(q), 10, C.byref(pp), None, ptr(labels), ptr(dist)), dist, labels)
    refused(lib.lm_pq_flat_search(idx._h, n, ptr(q), 10, C.byref(pp), None, ptr(labels), ptr(dist)), dist, labels)
    tab, i32, f32, u8 = np.zeros((8, 1536), np.float32), np.full(64, -77, np.int32), np.full(64, 123.25, np.float32), np.full(64, 0xEE, np.uint8)
    a, h = (lambda v: v.ctypes.data), C.c_void_p()
    assert lib.lm_index_create_view(8, 1536, 1, C.byref(_lib.GraphLevel(None, a(i32), 8, 4)), 1, 0, 0, C.byref(h)) == _lib.LM_EINVAL and not h.value
    refused(lib.lm_select_neighbors(a(tab), 0, 8, 1536, 1, a(i32), a(f32), 2, 4, 2, 1.0, a(u8), None), f32, i32)
    refused(lib.lm_graph_add_links(a(tab), 0, 1536, 1, a(i32), a(f32), a(i32), 8, 4, a(i32), a(i32), a(f32), 2, 1.0, a(u8), 64, None), f32, i32)
    refused(lib.lm_graph_prune_hubs(a(tab), 0, 1536, 1, a(i32), 8, 4, 2, 1, 1.0, a(i32), a(f32), a(i32), a(i32), a(i32), a(u8), 64, None), f32, i32)
    assert np.all(u8 == 0xEE)
    scenario(1536, L2, 1533, 1, 40).run(be, worlds=("persist_wg", "lock_wg"), idx=idx)  # the handle serves the next call
    idx.close()


# ---- the host build: 1536 and 4096 on a 150-node graph, a rotation through (metric, dtype) --------------------------------------------------
def case_search():
    for dp, metric, f16 in ((1536, IP, False), (4096, L2, True)):
        run_search(HostBackend(), dp, metric, 150, ds=(dp - 3,), f16s=(f16,), worlds=("persist_wg", "lock_wg"), beams=(4,))
    run_provider(HostBackend(), 1536, L2, 150, worlds=("rank_wg", "memo"))


def case_gather_and_exact():
    from leann_amd import _lib
    from tests import gpu_exact_util as xu

    for dp, metric, f16, npairs in ((1536, IP, True, 17), (4096, L2, False, 1), (4096, IP, False, 100)):
        tab, q, qidx, ids, exp = gather_case(dp, f16, npairs, metric)
        out = np.full(npairs + 8, np.nan, np.float32)
        rc = _lib.load().lm_dist_gather(tab.ctypes.data, int(f16), dp, metric, q.ctypes.data, qidx.ctypes.data, ids.ctypes.data, npairs, out.ctypes.data, None)
        assert rc == 0 and np.isnan(out[npairs:]).all() and np.array_equal(out[:npairs].view(np.uint32), exp.view(np.uint32)), (dp, metric, f16, npairs)
    for dp, ntable, nq, metric, f16, masked in ((1536, 1500, 9, IP, False, True), (4096, 1500, 9, L2, True, False), (4096, 1, 1, IP, False, False)):
        table, q, words, el, ed = exact_case(dp, ntable, nq, f16, metric, masked)
        rc, L, D, guards = xu.exact_host(_lib.load(), table, q, 10, metric, words)
        assert rc == 0 and guards and xu.same(L, D, el, ed), (dp, ntable, nq, metric, f16, masked)


def case_edges():
    run_envelope(HostBackend(), 150)
    run_refusals(HostBackend())


CASES = dict(search=case_search, gather_and_exact=case_gather_and_exact, edges=case_edges)

if __name__ == "__main__":
    _load(sys.argv[1])
    for name in sys.argv[2:] or list(CASES):
        CASES[name]()
        print(f"wide {name}: ok", flush=True)
    print("ALL CASES OK")
