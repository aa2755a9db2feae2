"""lm_pq_encode / lm_pq_train on the MI355X: codes byte for byte and codebooks bit for bit against the C restatement
(tests/pq_ref/lm_pq_ref.c) at the shapes the 10M configuration and the bench quantise at; the kernels' output attached with
lm_pq_attach and searched against the oracle; two runs of the training give the same bytes."""
import numpy as np
import pytest

from tests.util import clustered, oracle_graph, queries_near

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_():
    import torch

    from leann_amd import _lib

    _lib.require_gpu()
    return torch


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    from tests.pq_ref_util import compile_ref, load_ref

    return load_ref(compile_ref(tmp_path_factory.mktemp("pq_ref")))


@pytest.fixture(scope="module")
def corpus():
    return clustered(200_000, 384, 21, n_centers=2000, sigma=0.35)


def _sample_codebooks(x, d, offsets, seed):
    """256 rows of x as every chunk's centroids, uniform [m, 256, d/m] or the flat chunked layout."""
    rows = np.random.default_rng(seed).permutation(x.shape[0])[:256]
    flat = np.concatenate([x[rows, lo:hi].astype(np.float32).reshape(-1) for lo, hi in zip(offsets[:-1], offsets[1:])])
    return flat


@pytest.mark.parametrize("m,f16", [(96, False), (48, False), (96, True)])
def test_encode_matches_the_c_restatement(ref, torch_, corpus, m, f16):
    """200 000 x 384, the codebooks trained by lm_pq_train (2 iterations from 256 sampled rows): not one code differs."""
    torch = torch_
    from leann_amd.pq import encode_pq_kernel, lloyd_kernel
    from tests.pq_ref_util import ref_encode

    x = corpus.astype(np.float16) if f16 else corpus
    xd = torch.from_numpy(x).cuda()
    d = x.shape[1]
    off = np.arange(m + 1) * (d // m)
    init = torch.from_numpy(_sample_codebooks(x, d, off, 5).reshape(m, 256, d // m)).cuda()
    cb = lloyd_kernel(xd[:50_000], init, 2)
    got = encode_pq_kernel(xd, cb).cpu().numpy()
    exp = ref_encode(ref, x, d, cb.cpu().numpy())
    bad = int((got != exp).sum())
    print(f"encode m={m} f16={f16}: codes that differ: {bad} of {got.size}; distinct codes used: {len(np.unique(got))}")
    assert got.shape == (x.shape[0], m) and bad == 0


def test_encode_chunked_layout_matches_the_c_restatement(ref, torch_, corpus):
    """Unequal chunk lengths (1 .. 64, two empty chunks), 4 trailing dimensions without a code, rows taken from a padded fp32 table."""
    torch = torch_
    from leann_amd.pq import encode_pq_kernel
    from tests.pq_ref_util import ref_encode

    lens = [4] * 20 + [0, 8, 8, 16, 1, 3, 0, 64, 32, 12, 2, 2] + [6] * 25 + [2]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    assert off[-1] == 380
    table = torch.zeros((corpus.shape[0], 448), device="cuda")
    table[:, :384] = torch.from_numpy(corpus).cuda()
    cb = _sample_codebooks(corpus, 384, off, 6)
    got = encode_pq_kernel(table[:, :384], torch.from_numpy(cb).cuda(), chunk_offsets=off).cpu().numpy()
    exp = ref_encode(ref, corpus, 384, cb, off)
    bad = int((got != exp).sum())
    print(f"encode chunked m={len(lens)}: codes that differ: {bad} of {got.size}")
    assert got.shape == (corpus.shape[0], len(lens)) and bad == 0


def test_train_matches_the_c_restatement_and_is_deterministic(ref, torch_, corpus):
    """s = 131 072 x 384, m = 96, iters = 4: the codebooks equal the restatement's bit for bit, and a second run returns the same bytes."""
    torch = torch_
    from leann_amd.pq import lloyd_kernel
    from tests.pq_ref_util import ref_train

    xs = corpus[:131_072]
    off = np.arange(97) * 4
    init = _sample_codebooks(xs, 384, off, 7).reshape(96, 256, 4)
    xd = torch.from_numpy(xs).cuda()
    got = lloyd_kernel(xd, torch.from_numpy(init).cuda(), 4).cpu().numpy()
    again = lloyd_kernel(xd, torch.from_numpy(init).cuda(), 4).cpu().numpy()
    exp = ref_train(ref, xs, 384, init, 4)
    diff = int((got.view(np.uint32) != exp.view(np.uint32)).sum())
    print(f"train: codebook words that differ from the restatement: {diff} of {got.size}; moved from the start: {int((got != init).sum())}")
    assert got.tobytes() == again.tobytes()
    assert diff == 0 and (got != init).any()


def test_kernel_made_quantiser_plugs_into_the_pq_search(torch_):
    """30 000 x 128 trained and encoded by the kernels, attached with lm_pq_attach to a flat graph: lm_pq_batch_search returns the ids,
    distance bits and counts of orc_pq_search on the same codes (the comparison of tests/test_gpu_pq.py::test_pq_search_parity, case 1 and 3)."""
    torch = torch_
    from leann_amd.hnsw_builder import build_hnsw
    from leann_amd.index import Mi355xIndex
    from leann_amd.pq import encode_pq_kernel, flat_graph, train_pq_kernel
    from oracle import oracle as orc

    n, d, m = 30_000, 128, 32
    x = clustered(n, d, 8, n_centers=64, sigma=0.5)
    g = flat_graph(build_hnsw(x, "l2", M=12, ef_construction=60, seed=8), x)
    xd = torch.from_numpy(x).cuda()
    cbt = train_pq_kernel(xd, m, iters=6, seed=8)
    cb, codes = cbt.cpu().numpy(), encode_pq_kernel(xd, cbt).cpu().numpy()
    assert cb.shape == (m, 256, d // m) and codes.shape == (n, m) and len(np.unique(codes)) > 200
    q = queries_near(x, 40, 9)
    og = oracle_graph(g, d)
    idx = Mi355xIndex.from_csr(g)
    idx.set_stream(torch.cuda.current_stream().cuda_stream)
    idx.attach_pq(cb, codes)
    for L, W in ((32, 1), (64, 4)):
        oi, od, ost = orc.pq_search(og, cb, codes, q, 10, L=L, W=W, skip_search_reorder=True)
        gi, gd = idx.pq_search(q, 10, idx.make_pq_params(L, W, skip_search_reorder=True))
        st = idx.stats()
        assert np.array_equal(gi, oi) and np.array_equal(gd.view(np.uint32), od.view(np.uint32))
        assert st["ndis"] == ost["n_adc"] and st["nexpand"] == ost["n_expand"] and st["nrounds"] == ost["n_rounds"], (st, ost)
    idx.attach_table(x)
    oi, od, _ = orc.pq_search(og, cb, codes, q, 10, L=64, W=4, table=x)
    gi, gd = idx.pq_search(q, 10, idx.make_pq_params(64, 4))
    assert np.array_equal(gi, oi) and np.array_equal(gd.view(np.uint32), od.view(np.uint32))
    idx.close()


def test_backend_build_parameter_selects_the_kernels(torch_, tmp_path):
    """pq_bytes with gpu_pq_kernel=True: <stem>_pq.npz holds what the kernels return for the corpus, and the searcher opens it."""
    torch = torch_
    from leann_amd._compat import BACKEND_REGISTRY
    from leann_amd.backend import write_leann_bundle
    from leann_amd.pq import encode_pq_kernel, train_pq_kernel

    n = 3000
    x = clustered(n, 384, 34)
    p = str(tmp_path / "k.leann")
    write_leann_bundle(p, [f"passage {i}" for i in range(n)], x, "sentence-transformers/all-MiniLM-L6-v2", distance_metric="l2", M=8, efConstruction=40,
                       is_recompute=False, pq_bytes=48, gpu_pq_kernel=True)
    z = np.load(next(tmp_path.glob("*_pq.npz")))
    xd = torch.from_numpy(x).cuda()
    cb = train_pq_kernel(xd, 48, seed=0)
    assert z["codebooks"].tobytes() == cb.cpu().numpy().tobytes()
    assert np.array_equal(z["codes"], encode_pq_kernel(xd, cb).cpu().numpy())
    s = BACKEND_REGISTRY["mi355x"].searcher(p)
    r = s.search(x[:9] + 1e-4, 3, complexity=32, recompute_embeddings=False)
    assert [row[0] for row in r["labels"]] == [str(i) for i in range(9)]
    s.cleanup()
