"""lm_index_search_filtered (csrc/lm_filter_impl.h: k_filter_collect) on the MI355X: the cases of tests/emulated_filtered_cases.py -- every source
(provider with and without the per-call memo, a hub cache, fp32 / fp16 tables), the whole parameter grid, every allow-list form, ties / NaN /
the zero query / a seed without neighbours, the three invariants of include/leann_mi355x.h, the rejections on sentinel-filled buffers, the
wrappers -- and a pruned bundle WITHOUT PQ codes searched through Mi355xSearcher.search(graph_filter=True, allowed_ids=...).  Every comparison is
exact: labels, distance bits, stats, the provider's request lists and "filtered_allowed_evals" against the reference composed from the
unmodified oracle in tests/filtered_ref_util.py."""
import numpy as np
import pytest

from tests import emulated_filtered_cases as cases


def _has_gpu() -> bool:
    try:
        import torch

        return torch.cuda.is_available()
    except Exception:  # noqa: BLE001
        return False


pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not _has_gpu(), reason="needs an MI355X")]

_GRID = cases.parameter_grid(False)


@pytest.fixture(scope="module")
def gpu():
    from leann_amd import _lib
    from oracle import oracle as orc

    _lib.require_gpu()
    orc.lib()
    return cases.GpuBackend()


@pytest.mark.parametrize("name", ("ip64", "l2_100"))
def test_sources(gpu, name):
    """Provider at B = 1 (no memo), 3 and 70 (memo), memo off, hub cache, fp32 / fp16 table with "persistent_table" at its default."""
    cases.case_sources(gpu, (name,))


@pytest.mark.parametrize("ef", sorted({g[0] for g in _GRID}))
@pytest.mark.parametrize("name", ("ip64", "l2_100"))
def test_parameters(gpu, name, ef):
    """efSearch x k in {1, 10, 64} x beam in {1, 4} x batch_size in {0, 32}: k = 64 at efSearch 16, k = 1 with beam 4 and batch_size 32."""
    cases.case_parameters(gpu, [g for g in _GRID if g[0] == ef], name)


@pytest.mark.parametrize("name", ("ip64", "l2_100"))
def test_allow_lists(gpu, name):
    cases.case_allow_lists(gpu, (name,))


def test_ranking(gpu):
    cases.case_ranking(gpu)


@pytest.mark.parametrize("name", ("ip64", "l2_100"))
def test_invariants(gpu, name):
    """70 queries at max_batch 0 / 32 / 1 and alone, host and device entry, calls in a row, lm_index_search before and after."""
    cases.case_invariants(gpu, name)


def test_rejections_leave_the_outputs_untouched(gpu):
    cases.case_rejections(gpu)


def test_index_wrappers_and_backend_wiring(gpu):
    cases.case_wiring(gpu)


def test_graph_filter_on_a_pruned_bundle_without_pq_codes(tmp_path):
    """A recompute-mode searcher over a pruned bundle that has neither stored embeddings nor PQ codes: search(graph_filter=True, allowed_ids=10 %
    of the ids) returns only allowed labels, at least as many per query as post-filtering the plain graph search at the same complexity (and
    those first), the stats of the plain search, and more on at least one query."""
    import torch

    from leann_amd._compat import BACKEND_REGISTRY
    from leann_amd.backend import write_leann_bundle
    from leann_amd.encoder import BertEncoder
    from leann_amd.tokenizer import load_tokenizer

    n, k, ef = 500, 5, 32
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
    write_leann_bundle(p, texts, emb, model, distance_metric="mips", M=8, efConstruction=40)
    s = BACKEND_REGISTRY["mi355x"].searcher(p, allow_random_weights=True)
    assert s.is_pruned and not getattr(s, "_has_pq", False)
    allowed = set(int(v) for v in np.random.default_rng(3).permutation(n)[: n // 10])
    q = np.ascontiguousarray(emb[100:108])
    with pytest.raises(ValueError):
        s.search(q, k, recompute_embeddings=True, zmq_port=5557, allowed_ids=sorted(allowed))
    for kw in (dict(exact=True), dict(pq_flat=True)):
        with pytest.raises(ValueError):
            s.search(q, k, recompute_embeddings=True, zmq_port=5557, graph_filter=True, allowed_ids=sorted(allowed), **kw)
    plain = s.search(q, k, complexity=ef, recompute_embeddings=True, zmq_port=5557)
    st_plain = s.last_stats()
    kept = [[lab for lab in row if int(lab) in allowed] for row in plain["labels"]]
    r = s.search(q, k, complexity=ef, recompute_embeddings=True, zmq_port=5557, graph_filter=True, allowed_ids=sorted(allowed))
    st = s.last_stats()
    got = [[lab for lab in row if lab != "-1"] for row in r["labels"]]
    assert all(int(lab) in allowed for row in got for lab in row)
    assert all(g[: len(kr)] == kr for g, kr in zip(got, kept))
    assert sum(len(g) for g in got) > sum(len(kr) for kr in kept)
    assert all(int(st[f]) == int(st_plain[f]) for f in ("ndis", "nexpand", "nrounds", "nunique"))
    assert s.search(q, k, complexity=ef, recompute_embeddings=True, zmq_port=5557, graph_filter=True)["labels"] == plain["labels"]
    s.cleanup()
