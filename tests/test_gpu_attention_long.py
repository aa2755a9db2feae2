"""Head_dim-32 attention for sequences of 257..512 tokens (csrc/lm_attn_v3.hip: k_attn_varlen_hd32_long beside generation 3 in one launch)
through every entry point that takes such lengths, against plain torch in fp64 / fp32."""
import ctypes as C
import functools
import os
from unittest import mock

import numpy as np
import pytest
import torch

from leann_amd import _lib
from leann_amd.encoder import BertEncoder, EncoderConfig, fused_attention_hd32
from leann_amd.recompute import RecomputeProvider
from leann_amd.token_store import TokenStore

pytestmark = pytest.mark.gpu
LENS = [512, 257, 256, 33, 288, 1, 289, 511, 300, 180, 400, 64]  # 288 = exactly nine full tiles


def _cu(lens):
    return torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32).cuda()


def _randn(n, heads, g, scale=1.5):
    return (torch.randn((n, 96 * heads), generator=g) * scale).half()


def _ref(qkv, lens, heads):
    # softmax(Q K^T / sqrt 32) V per sequence and head in fp64; and the rows whose maximum over keys >= 256 exceeds tile 0's by > 8 log2 units
    q3, out, grew, a = qkv.double().view(-1, 3, heads, 32), [], 0, 0
    for n in lens:
        q, k, v = (q3[a:a + n, j].transpose(0, 1) for j in range(3))
        sc = q @ k.transpose(1, 2) / 32**0.5
        out.append((torch.softmax(sc, -1) @ v).transpose(0, 1).reshape(n, heads * 32))
        if n > 256:
            grew += int(((sc[:, :, 256:].max(-1).values - sc[:, :, :32].max(-1).values) * 1.4426950408889634 > 8.0).sum())
        a += n
    return torch.cat(out), grew


def _rows(lens, keep):
    off = np.concatenate([[0], np.cumsum(lens)])
    return torch.from_numpy(np.concatenate([np.arange(off[i], off[i + 1]) for i in range(len(lens)) if keep(lens[i])])).cuda()


@pytest.mark.parametrize("heads", [12, 2])
def test_long_launch_matches_fp64_and_short_sequences_keep_their_bits(heads):
    qkv = _randn(sum(LENS), heads, torch.Generator().manual_seed(heads)).cuda()
    out = fused_attention_hd32(qkv, _cu(LENS), heads, 512)
    assert out is not None and not torch.isnan(out).any()
    err = (out.double() - _ref(qkv, LENS, heads)[0]).abs().max().item()
    assert err < 6e-3, err  # generation 3's bound on these inputs: the long form rounds the same operands and sums in fp32
    assert all(torch.equal(out, fused_attention_hd32(qkv, _cu(LENS), heads, 512)) for _ in range(3))
    rows = _rows(LENS, lambda n: n <= 256)  # ... launched on their own: the same kernel, the same bits
    assert torch.equal(out[rows], fused_attention_hd32(qkv[rows].contiguous(), _cu([n for n in LENS if n <= 256]), heads, 256))


def test_a_unit_reads_its_own_tiles_only():
    g, got = torch.Generator().manual_seed(3), []
    fixed = {n: _randn(n, 12, g) for n in (300, 512)}
    for order in ([40, 300, 512], [512, 100, 257, 300, 7]):
        o = fused_attention_hd32(torch.cat([fixed[n] if n in fixed else _randn(n, 12, g) for n in order]).cuda(), _cu(order), 12, 512)
        got.append([o[_rows(order, lambda m: m == n)] for n in fixed])
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])


def test_rescale_branch_beyond_tile_eight():
    """Keys at positions >= 256 (one in the masked last tile of the 300-token sequence) whose scores exceed everything before them by far, for
    query rows below and above 256: the deferred maximum must be rescaled in the tiles only the long form has."""
    lens, H = [512, 300], 384
    qkv = _randn(812, 12, torch.Generator().manual_seed(5), 1.2).float()
    for tq, tk, h, gain in ((3, 300, 0, 3.0), (100, 511, 1, 4.0), (500, 257, 5, 3.5), (40, 420, 7, 3.0), (260, 330, 8, 3.0),
                            (512 + 10, 512 + 295, 2, 4.0), (512 + 290, 512 + 260, 3, 3.0), (512 + 200, 512 + 299, 11, 5.0)):
        qkv[tk, H + 32 * h: H + 32 * h + 32] = gain * qkv[tq, 32 * h: 32 * h + 32]
    qkv = qkv.half().cuda()
    ref, grew = _ref(qkv, lens, 12)
    assert grew >= 5
    o = fused_attention_hd32(qkv, _cu(lens), 12, 512)
    assert not torch.isnan(o).any() and (o.double() - ref).abs().max().item() < 5e-3


@functools.lru_cache(maxsize=None)
def _bge():
    # a two-layer model of bge-small's shape (hidden 384, CLS pooling, 512 positions) in fp16 on the GPU; 26 chunks, > 8192 tokens
    cfg = EncoderConfig(vocab_size=2000, hidden=384, layers=2, heads=12, ffn=384, max_pos=512, pooling="cls", normalize=True, max_seq_length=512)
    lens = np.array([512, 257, 300, 400, 511, 289, 450, 380] * 3 + [600, 120], dtype=np.int64)  # 600: truncated to 512
    tok = np.random.default_rng(1).integers(0, 2000, int(lens.sum())).astype(np.uint16)
    return cfg, BertEncoder.random_init(cfg, 0).to("cuda", dtype=torch.float16).eval(), tok, lens


def test_whole_forward_one_call_and_per_kernel(monkeypatch):
    cfg, enc, tok, lens = _bge()
    off, lens = np.concatenate([[0], np.cumsum(lens)]), np.minimum(lens, 512).astype(np.int32)
    ids = np.zeros((len(lens), 512), dtype=np.int32)
    for i, n in enumerate(lens):
        ids[i, :n] = tok[off[i]: off[i] + n]
    with torch.no_grad():
        ref = BertEncoder.random_init(cfg, 0).eval()(torch.from_numpy(ids), torch.from_numpy(lens)).float()  # the same weights, fp32, on the CPU
    used, real = [], _lib.check
    monkeypatch.setattr(_lib, "check", lambda rc, what="": (used.append(what), real(rc, what))[1])
    monkeypatch.setattr("torch.nn.attention.varlen.varlen_attn", lambda *a, **k: pytest.fail("torch's attention instead of the kernel"))
    one = enc.encode_tokens_packed(torch.from_numpy(ids).cuda(), torch.from_numpy(lens).cuda())
    assert "lm_bert_h384_forward_packed" in used and "lm_attn_varlen_hd32_f16" not in used, used
    assert (one.cpu() - ref).abs().max().item() <= 5e-3  # unit-norm embeddings
    used.clear()
    monkeypatch.setenv("LEANN_MI355X_ONECALL", "0")
    per = enc.encode_tokens_packed(torch.from_numpy(ids).cuda(), torch.from_numpy(lens).cuda())
    assert used.count("lm_attn_varlen_hd32_f16") == cfg.layers and "lm_bert_h384_forward_packed" not in used, used
    assert torch.equal(one, per)


def test_builtin_provider_equals_the_python_path_at_512():
    _, enc, tok, lens = _bge()
    ts = TokenStore(tok, np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64))
    nat, py = (RecomputeProvider(enc, ts, 384, torch.device("cuda")) for _ in range(2))
    assert nat.T == 512 and nat.native() is not None
    d_ids = torch.from_numpy(np.random.default_rng(2).permutation(len(lens)).astype(np.int32)).cuda()
    a = nat.embed_ids(d_ids)
    with mock.patch.dict(os.environ, {"LEANN_MI355X_NATIVE_PROVIDER": "0"}):
        assert py.native() is None
        b = py.embed_ids(d_ids)
    assert torch.equal(a, b), float((a - b).abs().max())
    assert nat.native_stats()["tokens"] == int(np.minimum(lens, 512).sum())
    nat.close()


@pytest.mark.parametrize("entry", ["lm_attn_varlen_hd32_f16", "lm_attn_varlen_f16", "lm_bert_h384_forward_packed", "lm_bert_forward_packed",
                                   "lm_recompute_create", "lm_recompute_create_general"])
def test_513_tokens_are_rejected_before_anything_is_launched(entry):
    lib, enc, p = _lib.load(), _bge()[1], lambda t: C.c_void_p(t.data_ptr())
    cu, out = _cu([513]), torch.full((513, 384), 7.0, device="cuda")
    pk = enc.onecall_model() if entry in ("lm_bert_h384_forward_packed", "lm_recompute_create") else enc.general_model()
    if entry.startswith("lm_attn"):
        qkv = torch.zeros((513, 1152), dtype=torch.float16, device="cuda")
        rc = getattr(lib, entry)(p(qkv), p(cu), 1, 12, *([32] if entry == "lm_attn_varlen_f16" else []), 513, p(out), None)
    elif entry.startswith("lm_bert"):
        tok, ws = torch.zeros(513, dtype=torch.int32, device="cuda"), torch.empty(1 << 24, dtype=torch.uint8, device="cuda")
        rc = getattr(lib, entry)(C.byref(pk["model"]), p(tok), p(tok), p(cu), 1, 513, 513, p(ws), ws.numel(), p(out), None)
    else:
        h, ts = C.c_void_p(), TokenStore(_bge()[2][:600], np.array([0, 600], dtype=np.uint64))
        rc = getattr(lib, entry)(C.byref(pk["model"]), ts._h, 513, 1 << 20, C.byref(h))
        assert h.value is None
    torch.cuda.synchronize()
    assert rc == _lib.LM_EINVAL and "512" in _lib.last_error() and bool((out == 7.0).all())
