"""The flat PQ scan and its rerank tail (csrc/lm_pq_flat_impl.h: k_pq_flat_scan, k_pq_flat_merge; lm_pq_scan, lm_pq_flat_search*) on the MI355X:
the cases of tests/emulated_pq_flat_cases.py at their full sizes -- every slicing regime, every table layout and compiled form of the row fetch,
ties across slices / NaN / the zero query, the allow-list forms, the index form through a provider and through fp32 / fp16 tables, the argument
envelope on pre-filled buffers -- and a pruned bundle searched through Mi355xSearcher.search(pq_flat=True, allowed_ids=...).  Every comparison
is exact: labels, distance bits, the provider's request list and the stats against the reference composed in tests/pq_flat_ref_util.py."""
import numpy as np
import pytest

from tests import emulated_pq_flat_cases as cases
from tests import pq_flat_ref_util as fu


def _has_gpu() -> bool:
    try:
        import torch

        return torch.cuda.is_available()
    except Exception:  # noqa: BLE001
        return False


pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not _has_gpu(), reason="needs an MI355X")]

_GRID = cases.slicing_grid(False)


@pytest.fixture(scope="module")
def gpu():
    from leann_amd import _lib

    _lib.require_gpu()
    return cases.GpuBackend()


@pytest.mark.parametrize("ntotal", sorted({g[0] for g in _GRID}))
def test_slicing(gpu, ntotal):
    """ntotal x nq in {1, 3, one more than a query tile} x L in {1, 10, 64, 1024}; 2048 rows are the plan's one-slice limit."""
    cases.case_slicing(gpu, [g for g in _GRID if g[0] == ntotal])


@pytest.mark.parametrize("layout", [lay[0] for lay in cases.LAYOUTS])
def test_layouts(gpu, layout):
    """m = 4 .. 128, one table per workgroup (m = 96) and several (m = 48), the chunked layout with a zero-length chunk and chunk_offsets[m] < d,
    both metrics, ldq > d; m = 16 also from a code array that starts 4 bytes off a 16-byte boundary."""
    cases.case_layouts(gpu, (layout,))


def test_ranking(gpu):
    cases.case_ranking(gpu)


def test_allow_list(gpu):
    cases.case_allow_list(gpu)


def test_argument_checking(gpu):
    cases.case_argument_checking(gpu)


def test_index_form(gpu):
    """Provider (ONE sorted unique request, stats), fp32 / fp16 tables, skip_search_reorder, host and device entry with the same bits, and
    with L >= the allowed rows the bits of lm_index_search_exact under the same allow-list."""
    cases.case_index(gpu)


def test_index_form_rejections_leave_the_outputs_untouched(gpu):
    """Every LM_EINVAL / LM_ESTATE case of lm_pq_flat_search and lm_pq_flat_search_device on sentinel-filled label and distance buffers."""
    cases.case_index_rejections(gpu)


def test_batch_search_is_what_it_was_before_the_tail_was_shared(gpu):
    """lm_pq_batch_search on the fixed small index: labels, distance bits and (ndis, nexpand, nrounds, nunique) as recorded at the parent commit
    (cases.BATCH_SEARCH_AT_PARENT: first labels row [125, 153, 191, 81, 58], stats [343, 76, 13, 23] through the provider, [343, 76, 13, 0]
    through the table)."""
    cases.case_batch_search_unchanged(gpu)


def test_scan_wrapper_and_backend_wiring(gpu):
    cases.case_wiring(gpu)


def test_filtered_search_on_a_pruned_bundle_returns_top_k_allowed_labels(tmp_path):
    """A recompute-mode searcher over a pruned bundle (no stored embeddings, PQ codes of 96 bytes): search(pq_flat=True, allowed_ids=1 % of the
    ids) returns top_k allowed labels -- those of the composed reference, reranked with the rows the searcher's own provider embeds for the same
    request list -- where the graph search followed by the post-filter returns fewer."""
    import torch

    from leann_amd._compat import BACKEND_REGISTRY
    from leann_amd.backend import write_leann_bundle
    from leann_amd.encoder import BertEncoder
    from leann_amd.tokenizer import load_tokenizer

    n, k, L = 500, 3, 64
    texts = [f"passage {i} " + " ".join(f"w{(i * 7 + j) % 50}" for j in range(12)) for i in range(n)]
    model = "sentence-transformers/all-MiniLM-L6-v2"
    p = str(tmp_path / "pruned.leann")
    enc = BertEncoder.load(model, allow_random=True).to("cuda", dtype=torch.float16)
    tok = load_tokenizer(model, 256, p, texts, enc.cfg.vocab_size, allow_stand_in=enc.weights_source == "random")
    seqs = tok.encode_batch(texts)
    ids = torch.zeros((n, max(len(s) for s in seqs)), dtype=torch.int32)
    for i, s in enumerate(seqs):
        ids[i, : len(s)] = torch.tensor(s, dtype=torch.int32)
    emb = enc.encode_tokens(ids.cuda(), torch.tensor([len(s) for s in seqs], dtype=torch.int32).cuda()).float().cpu().numpy()
    write_leann_bundle(p, texts, emb, model, distance_metric="mips", M=8, efConstruction=40, pq_bytes=96)
    s = BACKEND_REGISTRY["mi355x"].searcher(p, allow_random_weights=True)
    assert s.is_pruned
    allowed = np.sort(np.random.default_rng(3).permutation(n)[:5])  # 1 %
    q = np.ascontiguousarray(emb[100:104])
    with pytest.raises(ValueError):
        s.search(q, k, recompute_embeddings=True, zmq_port=5557, allowed_ids=[int(v) for v in allowed])
    graph = s.search(q, k, complexity=L, recompute_embeddings=True, zmq_port=5557)
    kept = [[lab for lab in row if int(lab) in set(allowed.tolist())] for row in graph["labels"]]
    assert min(len(row) for row in kept) < k  # what the reference's filter-after-search leaves
    r = s.search(q, k, complexity=L, recompute_embeddings=True, zmq_port=5557, pq_flat=True, allowed_ids=[int(v) for v in allowed])
    st = s.last_stats()
    assert all(len(row) == k and all(int(lab) in set(allowed.tolist()) for lab in row) for row in r["labels"])
    z = np.load(tmp_path / "pruned_pq.npz")
    mask = np.zeros(n, bool)
    mask[allowed] = True
    rows = s._provider.embed_ids(torch.from_numpy(allowed.astype(np.int32)).to("cuda")).float().cpu().numpy()  # the request list of the search: all five
    table = np.zeros((n, emb.shape[1]), np.float32)
    table[allowed] = rows[:, : emb.shape[1]]
    el, ed, union = fu.expected_search(z["codebooks"], z["codes"], emb, q, k, L, fu.IP, mask, table=table)
    assert np.array_equal(union, allowed)
    assert r["labels"] == [[str(int(v)) for v in row] for row in el]
    assert fu.same(el, r["distances"], el, ed)  # the same request list, the same rows: the same bits
    assert (int(st["ndis"]), int(st["nunique"]), int(st["nrounds"]), int(st["nexpand"])) == (5 * 4, 5, 1, 0)
    s.cleanup()
