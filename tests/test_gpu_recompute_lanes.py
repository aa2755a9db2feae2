"""GPU tests of the recompute provider's lanes (csrc/lm_recompute.hip: one forward of a round as 2 or 3 concurrent parts on streams of the
handle's own): every lane count returns the bits of one lane -- a chunk's embedding does not depend on its place in a forward, and every
part runs the kernels chosen for the whole.  The large-forward kernels run at every size here (LEANN_MI355X_SMALL_TOKENS=0) and a part
needs more than 1024 tokens, so calls of 6-10 k tokens split."""
import os
import time
from unittest import mock

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LANE_MIN = 1024
N_RAGGED = 300  # chunks 0 .. 299: lengths 0 .. 256; chunks 300 .. 359: one token each


@pytest.fixture(scope="module", autouse=True)
def large_kernels_at_every_size():
    with mock.patch.dict(os.environ, {"LEANN_MI355X_SMALL_TOKENS": "0"}):
        yield


@pytest.fixture(scope="module")
def world(large_kernels_at_every_size):
    import torch

    from leann_amd import _lib
    from leann_amd.encoder import BertEncoder, EncoderConfig
    from leann_amd.token_store import TokenStore

    _lib.require_gpu()
    rng = np.random.default_rng(7)
    lens = rng.integers(1, 257, N_RAGGED)
    lens[7], lens[11] = 0, 256  # one empty chunk, one of the longest
    lens = np.concatenate([lens, np.ones(60, np.int64)])
    off = np.zeros(lens.shape[0] + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    tok = rng.integers(1000, 30000, int(off[-1])).astype(np.uint16)
    cfg = EncoderConfig(vocab_size=30522, hidden=384, layers=2, heads=12, ffn=384, max_pos=512, max_seq_length=256)
    enc = BertEncoder.random_init(cfg, seed=3).to("cuda", dtype=torch.float16).eval()
    return {"torch": torch, "tokens": TokenStore(tok, off), "enc": enc, "lens": lens}


def _provider(w, enc=None, hidden=384, lanes=1, **kw):
    from leann_amd.recompute import RecomputeProvider

    p = RecomputeProvider(enc if enc is not None else w["enc"], w["tokens"], hidden, w["torch"].device("cuda"), **kw)
    assert p.native() is not None
    p.set_native_option("lane_min_tokens", LANE_MIN)
    p.set_native_option("lanes", lanes)
    assert p.get_native_option("lanes") == lanes and p.get_native_option("lane_min_tokens") == LANE_MIN
    return p


def _calls(w, id_lists, lanes, **kw):
    """The calls back to back on one handle (no host synchronisation of the test's between them: buffers are reused and grown across
    calls); returns the embeddings and the forwards each call launched: a forward split over the lanes counts once per part (option
    "parts"; the statistics' `forwards` counts it once, whatever the lane count)."""
    torch = w["torch"]
    p = _provider(w, lanes=lanes, **kw)
    outs, forwards = [], []
    for ids in id_lists:
        f0, u0 = p.get_native_option("parts"), p.native_stats()["forwards"]
        outs.append(p.embed_ids(torch.from_numpy(np.asarray(ids, np.int32)).cuda()))
        forwards.append(p.get_native_option("parts") - f0)
        assert p.native_stats()["forwards"] - u0 == (forwards[-1] if "LEANN_MI355X_FORWARD_TOKENS" in os.environ else min(forwards[-1], 1))
    torch.cuda.synchronize()
    outs = [o.clone() for o in outs]
    p.close()
    return outs, forwards


def _ragged_calls(w):
    """four calls of 6-10 k tokens, growing and shrinking, the empty and the longest chunk in the first"""
    rng = np.random.default_rng(1)
    calls = []
    for n in (56, 72, 48, 64):
        ids = rng.choice(N_RAGGED, n, replace=False)
        if not calls:
            ids[3], ids[20] = 7, 11
        assert 6000 <= int(w["lens"][ids].sum()) <= 11000
        calls.append(ids)
    return calls


def _assert_same_bits(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.shape == y.shape and bool((x == y).all()), float((x - y).abs().max())


@pytest.mark.parametrize("lanes", [2, 3])
def test_lanes_return_the_bits_of_one_lane_over_back_to_back_calls(world, lanes):
    calls = _ragged_calls(world)
    ref, f1 = _calls(world, calls, 1)
    got, fl = _calls(world, calls, lanes)
    assert f1 == [1] * 4 and fl == [lanes] * 4  # every call really ran as `lanes` parts
    _assert_same_bits(got, ref)
    assert float(ref[0].abs().max()) > 0 and not bool(ref[0][3].any())  # (the empty chunk pools to the zero vector)


@pytest.mark.parametrize("lanes", [2, 3])
def test_edge_shapes_equal_one_lane(world, lanes):
    rng = np.random.default_rng(2)
    long_first = np.concatenate([[11], np.arange(N_RAGGED, N_RAGGED + 40)])  # a 256-token chunk among 1-token chunks: an equal-token split
    long_last = long_first[::-1].copy()                                      # would leave the part in front of / behind it empty
    calls = [[5], [5, 9], rng.choice(N_RAGGED, 6, replace=False), long_first, long_last, [7], [7, 7, 7]]
    assert int(world["lens"][calls[2]].sum()) < LANE_MIN
    ref, f1 = _calls(world, calls, 1)
    got, fl = _calls(world, calls, lanes)
    _assert_same_bits(got, ref)
    assert fl == f1 == [1, 1, 1, 1, 1, 0, 0]  # nothing here is large enough to split (an all-empty call runs no forward)
    # the token budget (2048 tokens per forward) together with lanes: the budget's forwards go round-robin to the lanes, unsplit
    with mock.patch.dict(os.environ, {"LEANN_MI355X_FORWARD_TOKENS": "2048"}):
        big = _ragged_calls(world)
        ref, f1 = _calls(world, big, 1)
        got, fl = _calls(world, big, lanes)
    _assert_same_bits(got, ref)
    assert fl == f1 and min(f1) >= 3


def test_kernel_plan_is_taken_from_the_unsplit_forward(world):
    """Mean length below 216 overall (the projection + attention pair), above it in the first part (where a forward of its own would take
    the fused kernel): the parts run the whole's kernels."""
    lens = world["lens"][:N_RAGGED]
    long_ids = np.flatnonzero(lens >= 232)[:10]
    short_ids = np.flatnonzero((lens >= 8) & (lens <= 90))
    need = int(lens[long_ids].sum())
    # just enough short chunks to outweigh the long ones, the longest of them first: half of the total then falls into that chunk, and the
    # first part is exactly the long chunks
    short_ids = short_ids[: int(np.searchsorted(np.cumsum(lens[short_ids]), need, side="right")) + 1]
    short_ids = short_ids[np.argsort(-lens[short_ids], kind="stable")]
    ids = np.concatenate([long_ids, short_ids])
    cu = np.concatenate([[0], np.cumsum(lens[ids])])
    total = int(cu[-1])
    assert long_ids.shape[0] == 10 and need > LANE_MIN and total - need > LANE_MIN
    assert int(np.searchsorted(cu[1:], total // 2, side="right")) == 10  # the split point (lm_rc_parts.h) is the first short chunk
    assert total < 216 * ids.shape[0] and need >= 216 * long_ids.shape[0]
    ref, f1 = _calls(world, [ids], 1)
    got, f2 = _calls(world, [ids], 2)
    assert (f1, f2) == ([1], [2])
    _assert_same_bits(got, ref)


@pytest.mark.parametrize("lanes", [2, 3])
def test_general_width_lanes_return_the_bits_of_one_lane(world, lanes):
    torch = world["torch"]
    from leann_amd.encoder import BertEncoder, EncoderConfig

    cfg = EncoderConfig(vocab_size=30522, hidden=768, layers=2, heads=12, ffn=1536, max_pos=512, max_seq_length=256)
    enc = BertEncoder.random_init(cfg, seed=4).to("cuda", dtype=torch.float16).eval()
    calls = _ragged_calls(world)
    ref, f1 = _calls(world, calls, 1, enc=enc, hidden=768)
    got, fl = _calls(world, calls, lanes, enc=enc, hidden=768)
    assert f1 == [1] * 4 and fl == [lanes] * 4
    _assert_same_bits(got, ref)


def test_batched_search_with_two_lanes_equals_one_lane_and_the_python_provider():
    """2,000 chunks, 64 queries per call: labels, distance bits and the search's counts at 2 lanes are those of 1 lane; the search over
    the library-side provider with 2 lanes equals the one over the Python provider and the oracle (tests/test_gpu_native_provider.py)."""
    import torch

    from leann_amd.encoder import BertEncoder, EncoderConfig
    from leann_amd.gpu_graph_build import build_graph_gpu
    from leann_amd.index import Mi355xIndex
    from leann_amd.recompute import RecomputeProvider
    from leann_amd.synth import CorpusSpec, SyntheticCorpus
    from leann_amd.token_store import TokenStore
    from tests.test_gpu_native_provider import _search_native_vs_python_vs_oracle

    n, nq = 2000, 64
    c = SyntheticCorpus(CorpusSpec(n_chunks=n, n_topics=8))
    tok, off = c.chunks()
    cfg = EncoderConfig(vocab_size=30522, hidden=384, layers=2, heads=12, ffn=384, max_pos=512, max_seq_length=256)
    enc = BertEncoder.random_init(cfg, seed=3).to("cuda", dtype=torch.float16).eval()
    w = {"torch": torch, "tokens": TokenStore(tok, off), "enc": enc}
    nat, py = _provider(w), RecomputeProvider(enc, w["tokens"], 384, torch.device("cuda"))
    X = nat.embed_ids(torch.arange(n, dtype=torch.int32, device="cuda"))
    g = build_graph_gpu(X, "mips", M=12, ef_construction=60)
    qt, qo, _ = c.queries(nq)
    Q = RecomputeProvider(enc, TokenStore(qt, qo), 384, torch.device("cuda")).embed_ids(torch.arange(nq, dtype=torch.int32, device="cuda"))
    idx = Mi355xIndex.from_csr(g)
    idx.set_stream(torch.cuda.current_stream().cuda_stream)
    idx.set_provider(nat)
    assert idx.native_provider
    prm = idx.make_params(ef=40, beam=2, recompute=True)
    res = {}
    for lanes in (1, 2, 1, 2):  # (alternating: each setting also follows the other on the same buffers)
        nat.set_native_option("lanes", lanes)
        f0 = nat.get_native_option("parts")
        d, i = idx.search_device(Q, 10, prm)
        torch.cuda.synchronize()
        st = idx.stats()
        got = (i.clone(), d.clone(), int(st["nunique"]), int(st["ndis"]), int(st["nrounds"]))
        if lanes in res:
            assert torch.equal(res[lanes][0], got[0]) and torch.equal(res[lanes][1], got[1]) and res[lanes][2:5] == got[2:5]
        res[lanes] = got + (nat.get_native_option("parts") - f0,)
    assert torch.equal(res[1][0], res[2][0]) and torch.equal(res[1][1], res[2][1])
    assert res[1][2:5] == res[2][2:5]
    assert res[2][5] > res[1][5]  # rounds did run as two parts
    idx.close()
    nat.set_native_option("lanes", 2)
    _search_native_vs_python_vs_oracle(torch, nat, py, g, Q, 384, 40, 2, True)
    nat.close()


def test_kernel_timing_counts_overlapping_launches_once(world):
    """With two lanes the same kernel runs on two streams side by side: the summed milliseconds of the timing facility stay within the
    wall time of the call they were measured in (launches and work still add up over both parts)."""
    torch = world["torch"]
    from leann_amd import _lib

    ids = torch.arange(N_RAGGED, dtype=torch.int32, device="cuda")
    p = _provider(world, lanes=2)
    p.embed_ids(ids)  # grows the buffers
    torch.cuda.synchronize()
    _lib.kernel_timing_enable((1 << _lib.KT_COUNT) - 1)
    try:
        _lib.kernel_timing_read(reset=True)
        f0 = p.get_native_option("parts")
        t0 = time.perf_counter()
        p.embed_ids(ids)
        torch.cuda.synchronize()
        wall_ms = (time.perf_counter() - t0) * 1e3
        kt = _lib.kernel_timing_read(reset=True)
    finally:
        _lib.kernel_timing_enable(0)
    assert p.get_native_option("parts") - f0 == 2
    assert kt["lm::k_layer_tail_h384"]["launches"] == 4 and kt["lm::k_qkv_h384"]["launches"] == 4  # 2 layers x 2 parts
    total_ms = sum(v["ms"] for v in kt.values())
    print(f"kernel-timing sum {total_ms:.3f} ms within wall {wall_ms:.3f} ms")
    assert 0 < total_ms <= wall_ms
    p.close()
