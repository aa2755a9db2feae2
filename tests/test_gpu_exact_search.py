"""lm_exact_search on the MI355X: the shapes tests/emulated_exact_cases.py runs on the CPU emulation and those only the gfx950 build can get
wrong -- tables of 1 .. k + 1 rows, the three slicing regimes of the policy in include/leann_mi355x.h (1024 rows: one slice; 2048: two; 20 000:
twenty, the last of 544 rows), one query more than a tile of eight, k up to LM_EXACT_MAX_K, all nine padded widths, both metrics and dtypes.
Labels are compared for equality and distances bit for bit with oracle.bruteforce_topk (on the compacted sub-table when there is an allow-list);
every output lives in a guard-filled buffer (tests/gpu_exact_util.py).  Premises (ties at the k-th rank and across slices, -1 fills) are asserted
on the oracle's output, never on the kernel's."""
import numpy as np
import pytest

from tests import gpu_exact_util as xu


def _has_gpu() -> bool:
    try:
        import torch

        return torch.cuda.is_available()
    except Exception:  # noqa: BLE001
        return False


pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not _has_gpu(), reason="needs an MI355X")]

KS = (1, 10, 64, 256)
NQS = (1, 3, xu.QTILE + 1)
ONE_SLICE, TWO_SLICES, MANY_SLICES = 1024, 2048, 20000


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from leann_amd import _lib
    from oracle import oracle as orc

    _lib.require_gpu()
    orc.lib()


def _check(table, q, k, metric, mask=None, stray=False):
    words = None if mask is None else xu.bitmap(mask, stray)
    rc, L, D, guards = xu.exact_gpu(table, q, k, metric, words)
    el, ed = xu.expected(table, q, k, metric, mask)
    assert rc == 0 and guards, (rc, guards)
    assert xu.same(L, D, el, ed), (table.shape, q.shape[0], k, metric, str(table.dtype))
    return el, ed


def test_policy_names_the_three_regimes():
    assert xu.plan(ONE_SLICE, 1) == (1, 1024) and xu.plan(TWO_SLICES, 1) == (2, 1024) and xu.plan(MANY_SLICES, 1) == (20, 1024)
    assert MANY_SLICES - 19 * 1024 == 544 and xu.plan(MANY_SLICES, xu.QTILE + 1)[0] == 20
    from leann_amd import _lib

    assert _lib.load().lm_exact_search_workspace_bytes(MANY_SLICES, 3, 10) == 20 * 3 * 10 * 8


@pytest.mark.parametrize("metric", (0, 1))
@pytest.mark.parametrize("f16", (False, True))
def test_row_counts_query_counts_and_k(metric, f16):
    run = 0
    for k in KS:
        for n in sorted({1, 15, 17, 63, 65, max(k - 1, 1), k, k + 1, ONE_SLICE, TWO_SLICES, MANY_SLICES}):
            for nq in NQS:
                table, q = xu.gauss_case(n, (48, 96, 384)[run % 3], nq, 1000 + run, f16)
                el, _ = _check(table, q, k, metric)
                assert ((el == -1).sum(1) == max(0, k - n)).all()
                run += 1


@pytest.mark.parametrize("dp", xu.WIDTHS)
def test_every_padded_width(dp):
    for i, (metric, f16) in enumerate(((0, False), (1, True), (0, True), (1, False))):
        table, q = xu.gauss_case(1500, dp - 3, 3, 2000 + dp + i, f16)
        assert table.shape[1] == dp
        _check(table, q, 10, metric)


@pytest.mark.parametrize("metric", (0, 1))
def test_ties_across_slices_and_at_the_kth_rank(metric):
    for f16 in (False, True):
        table, q = xu.integer_case(MANY_SLICES, 48, 3, 60 + metric, f16)
        for k in (10, 64):
            el, ed = _check(table, q, k, metric)
            far = xu.expected(table, q, k + 1, metric)[1]
            assert (far[:, k - 1] == far[:, k]).any()  # a tie between ranks k and k + 1
            rows = xu.plan(MANY_SLICES, 3)[1]
            assert ((ed[:, :-1] == ed[:, 1:]) & (el[:, :-1] // rows != el[:, 1:] // rows)).any()  # tie pairs with ids in different slices


@pytest.mark.parametrize("metric", (0, 1))
def test_nan_row_and_exact_zero_inner_product(metric):
    table, q = xu.gauss_case(200, 48, 2, 78, False)
    table[17, 3] = np.nan
    table[50] = 0.0
    el, ed = _check(table, q, 200, metric)
    assert el[0, -1] == 17 and np.isinf(ed[0, -1])  # NaN ranks as +inf
    if metric == 0:
        assert ed[0, int(np.flatnonzero(el[0] == 50)[0])].view(np.uint32) == 0x80000000  # the -0 case: key +0, returned as -key_dist


@pytest.mark.parametrize("metric", (0, 1))
def test_allow_list(metric):
    rng = np.random.default_rng(3 + metric)
    for n, f16, nq in ((MANY_SLICES, False, 3), (333, True, xu.QTILE + 1), (TWO_SLICES + 7, True, 1)):
        table, q = xu.gauss_case(n, 48, nq, 500 + n, f16)
        _check(table, q, 10, metric, rng.random(n) < 0.5)
        few = np.zeros(n, bool)
        few[rng.permutation(n)[:6]] = True
        el, _ = _check(table, q, 10, metric, few)
        assert (el[:, 6:] == -1).all() and (el[:, :6] >= 0).all()  # fewer than k rows allowed: -1 fills
        el, _ = _check(table, q, 10, metric, np.zeros(n, bool))
        assert (el == -1).all()
        if n % 32:
            _check(table, q, 10, metric, rng.random(n) < 0.5, stray=True)  # stray high bits of the last word set
            _check(table, q, 256, metric, np.ones(n, bool), stray=True)


def test_empty_table_and_rejected_arguments():
    import torch

    from leann_amd import _lib

    q = xu.gauss_case(4, 64, 3, 1, False)[1]
    for metric in (0, 1):
        _check(np.zeros((0, 64), np.float32), q, 5, metric)
    lib = _lib.load()
    t = torch.zeros((8, 64), device="cuda")
    D = torch.full((30,), float("nan"), device="cuda")
    L = torch.full((30,), 7, dtype=torch.int64, device="cuda")
    ws = torch.full((4096,), 0xEE, dtype=torch.uint8, device="cuda")
    tq = torch.from_numpy(q).cuda()
    good = dict(dtype=0, n=8, dp=64, metric=0, nq=3, k=10, nb=4096)
    for over in (dict(dp=48), dict(dp=448), dict(dtype=2), dict(metric=3), dict(k=0), dict(k=257), dict(nq=-1), dict(n=-1), dict(n=2**31), dict(nb=239)):
        a = dict(good, **over)
        rc = lib.lm_exact_search(t.data_ptr(), a["dtype"], a["n"], a["dp"], a["metric"], tq.data_ptr(), a["nq"], a["k"], None, D.data_ptr(), L.data_ptr(), ws.data_ptr(), a["nb"], None)
        assert rc == _lib.LM_EINVAL, over
    torch.cuda.synchronize()
    assert torch.isnan(D).all() and (L == 7).all() and (ws == 0xEE).all()


@pytest.mark.parametrize("metric", ("mips", "l2"))
def test_index_level_search_exact(metric):
    import torch

    from leann_amd.hnsw_builder import build_hnsw
    from leann_amd.index import Mi355xIndex
    from tests.util import clustered

    n, d, m = 3000, 48, 0 if metric == "mips" else 1
    x = clustered(n, d, 5, n_centers=8, sigma=0.5)
    q = x[:9] + 0.01
    mask = np.random.default_rng(8).random(n) < 0.3
    g = build_hnsw(x, metric, M=8, ef_construction=40)
    idx = Mi355xIndex.from_csr(g)
    with pytest.raises(RuntimeError):  # LM_ESTATE: no table
        idx.search_exact(q, 5)
    idx.attach_table(x)  # fp32 host table, library-owned copy
    prm = idx.make_params(ef=48, beam=2, recompute=False)
    before = idx.search(q, 10, prm)
    D, L = idx.search_exact(q, 20)
    assert xu.same(L, D, *xu.expected(xu.pad64(x), xu.pad64(q), 20, m))
    D, L = idx.search_exact(q, 20, allowed=mask)
    assert xu.same(L, D, *xu.expected(xu.pad64(x), xu.pad64(q), 20, m, mask))
    after = idx.search(q, 10, prm)  # the exact search's workspace is apart from the graph search's
    assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
    h = torch.from_numpy(xu.pad64(x.astype(np.float16))).cuda()
    idx.attach_table(h)  # fp16 device table, borrowed
    e16 = xu.expected(xu.pad64(x.astype(np.float16)), xu.pad64(q), 20, m, mask)
    D, L = idx.search_exact(q, 20, allowed=np.flatnonzero(mask))
    assert xu.same(L, D, *e16)
    Dd, Ld = idx.search_exact_device(torch.from_numpy(q).cuda(), 20, allowed=torch.from_numpy(mask))
    assert xu.same(Ld.cpu().numpy(), Dd.cpu().numpy(), *e16)
    idx.close()


def test_exact_topk_kernel_has_the_shape_of_exact_topk_ip():
    import torch

    from leann_amd.exact import exact_topk_ip, exact_topk_kernel
    from tests.util import clustered

    x = clustered(5000, 96, 12, n_centers=16, sigma=0.5)
    q = x[:7] + 0.02
    v, i = exact_topk_kernel(torch.from_numpy(q).cuda(), torch.from_numpy(x).cuda(), 10)
    el, ed = xu.expected(xu.pad64(x), xu.pad64(q), 10, 0)
    assert xu.same(i.cpu().numpy(), v.cpu().numpy(), el, ed)
    v2, i2 = exact_topk_ip(torch.from_numpy(q).cuda(), torch.from_numpy(x).cuda(), 10)
    assert v.shape == v2.shape and i.shape == i2.shape and v.dtype == v2.dtype and i.dtype == i2.dtype


def test_plugin_exact_and_allowed_ids(tmp_path):
    from leann_amd._compat import BACKEND_REGISTRY
    from leann_amd.backend import write_leann_bundle
    from tests.util import clustered

    n = 1500
    x = clustered(n, 384, 31)
    q = x[:5] + 1e-3
    p = str(tmp_path / "full.leann")
    write_leann_bundle(p, [f"passage {i}" for i in range(n)], x, "sentence-transformers/all-MiniLM-L6-v2", distance_metric="l2", M=8, efConstruction=40, is_recompute=False)
    s = BACKEND_REGISTRY["mi355x"].searcher(p)
    r = s.search(q, 8, recompute_embeddings=False, exact=True)
    el, ed = xu.expected(x, q, 8, 1)
    assert r["labels"] == [[str(int(v)) for v in row] for row in el] and xu.same(el, r["distances"], el, ed)
    allowed = [int(v) for v in np.random.default_rng(2).permutation(n)[:5]]
    mask = np.zeros(n, bool)
    mask[allowed] = True
    r = s.search(q, 8, recompute_embeddings=False, exact=True, allowed_ids=allowed)
    el, ed = xu.expected(x, q, 8, 1, mask)
    assert (el[:, 5:] == -1).all()
    assert r["labels"] == [[str(int(v)) for v in row] for row in el] and xu.same(el, r["distances"], el, ed)
    with pytest.raises(ValueError):
        s.search(q, 8, recompute_embeddings=False, allowed_ids=allowed)
    s.cleanup()
