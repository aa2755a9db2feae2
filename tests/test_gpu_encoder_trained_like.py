"""Every form of the encoder forward on a TRAINED-SHAPED model (tests/encoder_ref_util.py: sharp attention, GELU inputs out to +-7, LayerNorm
outliers, every parameter tensor different) against an fp64 reference of the same weights, the sensitivity of the result to every single
parameter tensor, the GELU of both kernels over the whole fp16 range, and the layer tail's one-pass variance on rows with a large mean.

The bound of the composed forward is measured, not chosen: E0 = max |first generation - fp64| (library GEMMs, torch attention, torch pooling
on the same fp16 weights: the same rounding points), every hand-written form within 2 x E0 and cosine >= 0.9999."""

# Measured on an MI355X (max |form - fp64| on unit-norm embeddings, 12 sequences of 1 .. 256 tokens, MiniLM-L6 shape):
#   form                                              max |diff|   x E0    min cosine
#   E0: first generation (library GEMMs, torch ops)   6.341e-04    1.00    0.9999983
#   1 small (general kernels in the one call)         4.360e-04    0.69    0.9999982
#   2 head-major pair + layer tail                    3.836e-04    0.60    0.9999986
#   3 fused QKV + attention + layer tail              7.099e-04    1.12    0.9999986
#   4 QKV from lm_gemm_f16 + attention + layer tail   3.280e-04    0.52    0.9999986
#   5 row-major lm_qkv_h384_f16 + attention + tail    3.836e-04    0.60    0.9999986   (the bits of form 2)
#   6 per-kernel launch path of 1 .. 5                the bits of the one call
#   7 native provider, default / SMALL_TOKENS=0       4.360e-04 / 3.836e-04            (the bits of forms 1 / 2)
#   8 hidden 768 (2 layers, ffn 3072), CLS            2.260e-04    1.08    0.9999990   (E0 2.090e-04)
#     hidden 768, mean pooling                        1.008e-04    1.13    0.9999998   (E0 8.952e-05)
# GELU epilogue of lm_gemm_f16 over all 63 488 finite fp16 inputs: max |diff| 9.763e-04 (half an ulp at |x| ~ 2^15), largest |diff| - (1e-6 + ulp / 2)
#   -4.72e-07, at most 0.596 ulp for x > -3, x for x >= 6, +-0 below -9: figure for figure what the numpy restatement of the polynomial gives.
# Layer-tail GELU sweep (inline-asm form): largest diff / bound 0.986, 0.983, 0.979, 0.995 in the four launches (the bound is half an fp16 ulp of the
#   output + 1 %: a value one ulp off anywhere in the row is outside), the same bits in four launches.
# One-pass variance of the layer tail, max |diff| / scale (tolerance 1.2e-2) with the rows of LayerNorm 1 / LayerNorm 2 at mean / std
#   0: 3.9e-4 / 3.9e-4   2: 3.9e-4 / 3.9e-4   8: 6.0e-4 / 3.8e-4   32: 5.8e-4 / 3.5e-4   64: 6.9e-4 / 9.3e-4   120: 7.1e-4 / 1.6e-3 (the cases below);
#   from calls of _variance_case by hand: 250: 1.6e-3 / 8.6e-3   400: 3.5e-3 / 2.2e-2   1000: 2.4e-2 / 1.7e-1.  fp16 level is 3.9e-4: LayerNorm 1 is at
#   1.5 x from mean/std 8 and 1.8 x at 64 .. 120, LayerNorm 2 at fp16 level up to 32, 2.4 x at 64, 4 x at 120; both grow with the square beyond.
import os
from unittest import mock

import numpy as np
import pytest

from tests import encoder_ref_util as U


def _has_gpu() -> bool:
    try:
        import torch

        return torch.cuda.is_available()
    except Exception:  # noqa: BLE001
        return False


pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not _has_gpu(), reason="needs an MI355X")]

# the first-generation encoder path (tests/test_gpu_encoder_kernels.py): library GEMMs, torch attention / pooling / packing
FIRST_GENERATION = {"LEANN_MI355X_ATTN": "0", "LEANN_MI355X_LN": "1", "LEANN_MI355X_POOL": "0", "LEANN_MI355X_EMBED": "0",
                    "LEANN_MI355X_PACK": "0", "LEANN_MI355X_LINEAR": "0", "LEANN_MI355X_GEMM": "0"}
LENGTHS = [256, 255, 224, 129, 33, 32, 2, 1, 180, 97, 64, 200]
L = 6
# form -> (environment, launches per kernel inside the ONE library call, _lib.check names of the per-kernel launch path)
FORMS = {
    "small": ({}, {"gemm_f16": 4 * L, "attn_varlen": L}, {"lm_gemm_f16": 4 * L, "lm_attn_varlen_hd32_f16": L, "lm_add_layernorm_f16": 2 * L}),
    "pair": ({"LEANN_MI355X_SMALL_TOKENS": "0"}, {"qkv_h384": L, "attn_varlen": L, "layer_tail_h384": L},
             {"lm_qkv_h384_f16": L, "lm_attn_varlen_hd32_f16": L, "lm_layer_tail_h384_f16": L}),
    "fused": ({"LEANN_MI355X_SMALL_TOKENS": "0", "LEANN_MI355X_FUSED_QKV_ATTN": "1"}, {"qkv_attn_h384": L, "layer_tail_h384": L},
              {"lm_qkv_attn_h384_f16": L, "lm_layer_tail_h384_f16": L}),
    "qkv_gemm": ({"LEANN_MI355X_SMALL_TOKENS": "0", "LEANN_MI355X_QKV_GEMM_TOKENS": "1000000"}, {"gemm_f16": L, "attn_varlen": L, "layer_tail_h384": L},
                 {"lm_gemm_f16": L, "lm_attn_varlen_hd32_f16": L, "lm_layer_tail_h384_f16": L}),
    "row_major": ({"LEANN_MI355X_SMALL_TOKENS": "0", "LEANN_MI355X_QKV_LAYOUT": "0"}, {"qkv_h384": L, "attn_varlen": L, "layer_tail_h384": L},
                  {"lm_qkv_h384_f16": L, "lm_attn_varlen_hd32_f16": L, "lm_layer_tail_h384_f16": L}),
}
KERNELS = ("layer_tail_h384", "gemm_ws_h384", "attn_varlen", "gemm_f16", "qkv_h384", "qkv_attn_h384")
# what lm_h384_first_half_form answers under the form's switches (0 fused, 1 head-major pair, 2 row-major pair); the small form has no first half of
# that kind and the qkv_gemm form overrides the answer inside the forward
FIRST_HALF = {"pair": 1, "fused": 0, "row_major": 2}
CHECK_NAMES = ("lm_bert_h384_forward_packed", "lm_bert_forward_packed", "lm_gemm_f16", "lm_gemm_ws_h384_f16", "lm_qkv_h384_f16", "lm_qkv_attn_h384_f16",
               "lm_attn_varlen_hd32_f16", "lm_attn_varlen_f16", "lm_layer_tail_h384_f16", "lm_add_layernorm_f16")


def _run(fn, env=None):
    """fn() under exactly the LEANN_MI355X_* switches of ``env`` -> (result, {check name: count}, {kernel: launches inside the library})."""
    import torch

    from leann_amd import _lib

    e = {k: v for k, v in os.environ.items() if not k.startswith("LEANN_MI355X_")}
    e.update(env or {})
    used = []
    real = _lib.check

    def recording(rc, what=""):
        used.append(what)
        return real(rc, what)

    _lib.kernel_timing_read(reset=True)
    _lib.kernel_timing_enable((1 << _lib.KT_COUNT) - 1)
    try:
        with mock.patch.dict(os.environ, e, clear=True), mock.patch.object(_lib, "check", new=recording), torch.no_grad():
            out = fn()
        torch.cuda.synchronize()
        kt = _lib.kernel_timing_read(reset=True)
    finally:
        _lib.kernel_timing_enable(0)
    return out, {n: used.count(n) for n in CHECK_NAMES if n in used}, {k: kt["lm::k_" + k]["launches"] for k in KERNELS if kt["lm::k_" + k]["launches"]}


def _bound(tag, got, ref, e0):
    err, cos = U.errors(got, ref)
    print(f"{tag}: max|diff| vs fp64 {err:.3e} ({err / e0:.2f} x E0 = {e0:.3e}), min cosine {cos:.7f}", flush=True)
    assert np.isfinite(err) and err <= 2.0 * e0 and cos >= 0.9999, (tag, err, e0, cos)


@pytest.fixture(scope="module")
def world():
    import torch

    cfg = U.minilm_cfg()
    enc = U.trained_like_init(cfg, 0).to("cuda", dtype=torch.float16).eval()
    ids, lens = U.make_batch(cfg, LENGTHS, 1)
    ref = U.reference_fp64(enc, ids, lens)  # of the fp16 weights the GPU model holds: rounding the weights is not part of any error below
    ti, tl = ids.cuda(), lens.cuda()
    first, _, kt = _run(lambda: enc.encode_tokens_packed(ti, tl), FIRST_GENERATION)
    assert not kt, kt  # no hand-written MFMA kernel in the yardstick
    e0, cos0 = U.errors(first, ref)
    print(f"E0 (first generation vs fp64): {e0:.3e}, min cosine {cos0:.7f}", flush=True)
    assert cos0 >= 0.9999
    return {"torch": torch, "cfg": cfg, "enc": enc, "ids": ids, "lens": lens, "ti": ti, "tl": tl, "ref": ref, "e0": e0}


@pytest.mark.parametrize("form", list(FORMS))
def test_every_form_of_the_forward_against_fp64(world, form):
    """The one library call in each of its five launch sequences (which kernels ran: the library's own launch counters), within 2 x E0 of fp64;
    the per-kernel launch path of the same switches (which kernels ran: the recorded _lib.check names) returns the same bits."""
    torch, enc, ti, tl = world["torch"], world["enc"], world["ti"], world["tl"]
    env, want_kernels, want_names = FORMS[form]
    if form in FIRST_HALF:  # the library's own decision for this batch under these switches: tells the head-major pair from the row-major one
        from leann_amd import _lib

        n_tok, n_seq = int(world["lens"].sum()), len(LENGTHS)
        assert _run(lambda: _lib.load().lm_h384_first_half_form(12, 256, n_tok, n_seq), env)[0] == FIRST_HALF[form], form
    one, names, kernels = _run(lambda: enc.encode_tokens_packed(ti, tl), env)
    assert names == {"lm_bert_h384_forward_packed": 1}, names
    assert kernels == want_kernels, (form, kernels)
    _bound(f"form {form}", one, world["ref"], world["e0"])
    per, names, _ = _run(lambda: enc.encode_tokens_packed(ti, tl), {**env, "LEANN_MI355X_ONECALL": "0"})
    assert "lm_bert_h384_forward_packed" not in names and {k: names.get(k, 0) for k in want_names} == want_names, (form, names)
    if form != "small":
        assert "lm_add_layernorm_f16" not in names and ("lm_gemm_f16" in names) == (form == "qkv_gemm"), names
    assert torch.equal(one, per), float((one - per).abs().max())
    again, _, _ = _run(lambda: enc.encode_tokens_packed(ti, tl), env)
    assert torch.equal(one, again)


@pytest.mark.parametrize("form", ["small", "pair"])
def test_native_recompute_provider_against_fp64(world, form):
    """RecomputeProvider.embed_ids over a TokenStore of the same sequences, library-side provider (lm_recompute_create + lm_recompute_embed): against
    fp64, not only against the Python provider -- and equal to the one-call forward of the same form bit for bit."""
    torch, enc = world["torch"], world["enc"]
    from leann_amd.recompute import RecomputeProvider
    from leann_amd.token_store import TokenStore

    seqs = [world["ids"][i, : int(n)].tolist() for i, n in enumerate(world["lens"])]
    store = TokenStore.from_lists(seqs)
    prov = RecomputeProvider(enc, store, 384, torch.device("cuda"))
    env, want_kernels, _ = FORMS[form]
    ids = torch.arange(len(seqs), dtype=torch.int32, device="cuda")
    got, names, kernels = _run(lambda: prov.embed_ids(ids), env)
    assert names.get("lm_bert_h384_forward_packed", 0) == 0 and prov.native_stats()["forwards"] == 1 and prov.native_stats()["chunks"] == len(seqs), (names, prov.native_stats())
    assert kernels == want_kernels, kernels
    _bound(f"native provider, form {form}", got, world["ref"], world["e0"])
    one, _, _ = _run(lambda: enc.encode_tokens_packed(world["ti"], world["tl"]), env)
    assert torch.equal(got, one)
    prov.close()
    store.close()


@pytest.mark.parametrize("pooling", ["cls", "mean"])
def test_hidden_768_forward_against_fp64(pooling):
    """lm_bert_forward_packed (general kernels, head_dim 64) on a trained-shaped 768-wide model, one sequence beyond 256 tokens."""
    import torch

    from leann_amd.encoder import EncoderConfig

    cfg = EncoderConfig(vocab_size=2000, hidden=768, layers=2, heads=12, ffn=3072, max_pos=512, max_seq_length=512, pooling=pooling)
    enc = U.trained_like_init(cfg, 3).to("cuda", dtype=torch.float16).eval()
    ids, lens = U.make_batch(cfg, [389, 64, 33, 1, 130, 17, 256], 2)
    ref = U.reference_fp64(enc, ids, lens)
    ti, tl = ids.cuda(), lens.cuda()
    first, _, kt = _run(lambda: enc.encode_tokens_packed(ti, tl), FIRST_GENERATION)
    assert not kt, kt
    e0, cos0 = U.errors(first, ref)
    print(f"hidden 768 {pooling}: E0 {e0:.3e}, min cosine {cos0:.7f}", flush=True)
    one, names, kernels = _run(lambda: enc.encode_tokens_packed(ti, tl))
    assert names == {"lm_bert_forward_packed": 1} and kernels == {"gemm_f16": 4 * cfg.layers, "attn_varlen": cfg.layers}, (names, kernels)
    _bound(f"hidden 768 {pooling}", one, ref, e0)
    per, names, _ = _run(lambda: enc.encode_tokens_packed(ti, tl), {"LEANN_MI355X_ONECALL": "0"})
    assert names.get("lm_gemm_f16") == 4 * cfg.layers and names.get("lm_attn_varlen_f16") == cfg.layers and "lm_bert_forward_packed" not in names, names
    assert torch.equal(one, per)


# ---- parameter sensitivity ------------------------------------------------------------------------------------------------------------
# (tensor, layer): the 12 tensors of a layer spread over layers 0 .. 5, the embedding LayerNorm, the type row, the position table
SENSITIVITY = [(n, i % L) for i, n in enumerate(U.LAYER_TENSORS)] + [("ln.weight", None), ("ln.bias", None), ("tok_type.weight", None), ("pos.weight", None)]


@pytest.fixture(scope="module")
def base_outputs(world):
    enc, ti, tl = world["enc"], world["ti"], world["tl"]
    return {f: _run(lambda: enc.encode_tokens_packed(ti, tl), FORMS[f][0])[0].clone() for f in ("small", "pair")}


@pytest.mark.parametrize("name,layer", SENSITIVITY, ids=[f"{n}-{l}" for n, l in SENSITIVITY])
def test_one_changed_parameter_tensor_changes_the_result_as_in_fp64(world, base_outputs, name, layer):
    """tensor.add_(delta) on ONE parameter tensor of the GPU model (0.3 N for vectors and embedding tables, 0.3 N x the tensor's own spread for the
    weight matrices): the default one-call forward and the large form meet the 2 x E0 bound against the fp64 reference OF THE CHANGED WEIGHTS, E0 being
    the first-generation path on the same inputs and the same changed weights, and moved by more than that bound -- a swapped, shared or dropped field,
    or a packed copy that was not rebuilt, fails one or the other.  The tensor is put back afterwards (another in-place change: another rebuild) and
    the first result must come back bit for bit.

    Inputs: the module's 12 sequences.  On six sequences of at most 64 tokens (lengths 64, 63, 33, 32, 2, 1) the maximum over 6 x 384 values is too
    noisy a yardstick: E0 of the 16 steps ranged from 1.7e-4 to 6.5e-4, the small form sat at 0.7 to 1.8 x E0 -- and at 2.06 x with out.bias of layer 3
    changed (8.3e-4 against 4.0e-4, one row of 33 tokens; every other row within 1.6 x of its first-generation figure).  Bisected through the
    per-kernel path against the fp64 activations: the small form's rms error is 9 to 20 % above the first generation's at EVERY layer (7.7e-4 against
    7.1e-4 behind layer 0, 1.9e-3 against 1.6e-3 behind layer 5; embeddings 7.9e-5 against 6.7e-5), no layer adds a step -- the general kernels' documented
    extra roundings (Q a second time after the softmax scale, the fp16 residual add of the GEMM epilogue), not a wiring fault; the large form is at or
    below the first generation at every layer.  On the 12 sequences the same 16 steps measure 0.59 to 1.77 x E0 (small) and 0.46 to 1.27 x (large)."""
    torch, enc = world["torch"], world["enc"]
    ids, lens, ti, tl = world["ids"], world["lens"], world["ti"], world["tl"]
    p = dict(enc.named_parameters())[name if layer is None else f"layers.{layer}.{name}"]
    g = torch.Generator(device="cpu").manual_seed(1000 + SENSITIVITY.index((name, layer)))
    delta = 0.3 * torch.randn(p.shape, generator=g) * (float(p.detach().float().std()) if (p.dim() == 2 and layer is not None) else 1.0)
    keep = p.detach().clone()
    run = lambda env: _run(lambda: enc.encode_tokens_packed(ti, tl), env)[0].clone()  # noqa: E731
    try:
        with torch.no_grad():
            p.add_(delta.to(p.device, p.dtype))
        ref = U.reference_fp64(enc, ids, lens)
        e0, _ = U.errors(run(FIRST_GENERATION), ref)
        for form in ("small", "pair"):
            got = run(FORMS[form][0])
            _bound(f"{name} (layer {layer}) changed, form {form}", got, ref, e0)
            moved = float((got - base_outputs[form]).abs().max())
            print(f"    moved by {moved:.3e}", flush=True)
            assert moved > 2.0 * e0, (name, layer, form, moved, e0)
    finally:
        with torch.no_grad():
            p.copy_(keep)
    for form in ("small", "pair"):
        assert torch.equal(run(FORMS[form][0]), base_outputs[form]), (name, form)


# ---- GELU -----------------------------------------------------------------------------------------------------------------------------
def test_gelu_of_the_general_gemm_over_every_finite_fp16_input():
    """lm_gemm_f16 with the GELU epilogue, W = identity, bias 0: the pre-activation IS x, for all 63 488 finite fp16 values (248 rows of 256)."""
    import torch

    from leann_amd.encoder import GEMM_EPI_GELU, fused_gemm

    x16 = U.all_finite_fp16()
    assert x16.shape[0] == 63488
    lin = torch.nn.Linear(256, 256)
    with torch.no_grad():
        lin.weight.copy_(torch.eye(256))
        lin.bias.zero_()
    lin = lin.to("cuda", dtype=torch.float16)
    x = torch.from_numpy(x16.copy()).view(248, 256).cuda()
    with torch.no_grad():
        got = fused_gemm(x, lin, GEMM_EPI_GELU)
        again = fused_gemm(x, lin, GEMM_EPI_GELU)
    torch.cuda.synchronize()
    assert got is not None and got.dtype == torch.float16 and torch.equal(got.view(torch.int16), again.view(torch.int16))
    rep = U.gelu_sweep_report(x16, got.cpu().numpy().reshape(-1))
    print("GELU epilogue of lm_gemm_f16 over every finite fp16 input:", rep, flush=True)
    U.assert_gelu_sweep(rep)


def _tail_layer(torch, ffn):
    from leann_amd.encoder import EncoderConfig, _Layer

    return _Layer(EncoderConfig(hidden=384, layers=1, heads=12, ffn=ffn)).to("cuda", dtype=torch.float16)


def test_gelu_of_the_layer_tail_over_a_sweep_of_pre_activations():
    """The layer tail's GELU (inline-asm micro-operations on the GPU) in isolation: attention, residual, W_o, b_o, beta1 = 0 make x1 exactly 0; W1 = 0 makes
    the pre-activation of hidden unit u exactly b1[u] (a sweep of [-9.5, 9.5] + the fp16 extremes); W2 routes unit 384 s + c to output feature c
    (launch s of four), b2 = 0, LayerNorm2 = plain normalisation.  Reference and bound: tests/encoder_ref_util.py: tail_gelu_reference."""
    import torch

    from leann_amd.encoder import fused_attn_out_mlp

    sweep = U.tail_gelu_sweep()
    layer = _tail_layer(torch, 1536)
    with torch.no_grad():
        for t in (layer.out.weight, layer.out.bias, layer.ln1.bias, layer.fc1.weight, layer.fc2.weight, layer.fc2.bias, layer.ln2.bias):
            t.zero_()
        layer.ln1.weight.fill_(1.0)
        layer.ln2.weight.fill_(1.0)
        layer.fc1.bias.copy_(torch.from_numpy(sweep.copy()))
    assert np.array_equal(layer.fc1.bias.detach().cpu().numpy(), sweep)
    tokens = 70  # two full 32-row blocks and a partial one
    a = torch.zeros((tokens, 384), dtype=torch.float16, device="cuda")
    res = torch.zeros_like(a)
    worst = 0.0
    for s in range(4):
        w2 = torch.zeros((384, 1536), dtype=torch.float16)
        w2[torch.arange(384), 384 * s + torch.arange(384)] = 1.0
        with torch.no_grad():
            layer.fc2.weight.copy_(w2)
            outs = [fused_attn_out_mlp(a, res, layer) for _ in range(4)]
        torch.cuda.synchronize()
        assert outs[0] is not None and all(torch.equal(outs[0].view(torch.int16), o.view(torch.int16)) for o in outs[1:]), s
        got = outs[0].float().cpu().numpy().astype(np.float64)
        assert np.isfinite(got).all(), s
        assert (got == got[0:1]).all(), s  # every token row is the same row
        ref, bound = U.tail_gelu_reference(sweep[384 * s: 384 * (s + 1)])
        d = np.abs(got[0] - ref)
        ratio = float((d / bound).max())
        worst = max(worst, ratio)
        print(f"layer-tail GELU sweep, launch {s}: max|diff| {d.max():.3e}, max diff / bound {ratio:.3f} (at b1 = {float(sweep[384 * s + int((d / bound).argmax())])})", flush=True)
        assert (d <= bound).all(), (s, ratio)
    print(f"layer-tail GELU sweep: worst diff / bound {worst:.3f}", flush=True)


# ---- the one-pass variance of the layer tail ---------------------------------------------------------------------------------------------
def _variance_case(ratio: float, which: str):
    """lm_layer_tail_h384_f16 (ffn 192, random weights, 300 tokens) on rows whose pre-LayerNorm sums have mean / std = ``ratio``: a constant added to
    b_o (which = "ln1": the sums resid + attn W_o^T + b_o) or to b_2 ("ln2": x + FC2 + b_2).  -> (max |diff| vs fp64, scale, measured mean / std)."""
    import torch
    import torch.nn.functional as F

    from leann_amd.encoder import fused_attn_out_mlp

    torch.manual_seed(300 + 192)
    layer = _tail_layer(torch, 192)
    with torch.no_grad():
        for ln in (layer.ln1, layer.ln2):
            ln.weight.copy_(1 + 0.1 * torch.randn(384))
            ln.bias.copy_(0.1 * torch.randn(384))
        layer.out.bias.copy_(0.2 * torch.randn(384))
        layer.fc1.bias.copy_(0.2 * torch.randn(192))
        layer.fc2.bias.copy_(0.2 * torch.randn(384))
    a = torch.randn((300, 384), device="cuda").half()
    res = torch.randn((300, 384), device="cuda").half()

    def reference():
        d = lambda t: t.detach().double().cpu()  # noqa: E731
        v1 = d(res) + d(a) @ d(layer.out.weight).t() + d(layer.out.bias)
        x1 = F.layer_norm(v1, (384,), d(layer.ln1.weight), d(layer.ln1.bias), layer.ln1.eps).half().double()  # the kernel keeps x as fp16 fragments
        v2 = x1 + F.gelu(x1 @ d(layer.fc1.weight).t() + d(layer.fc1.bias)) @ d(layer.fc2.weight).t() + d(layer.fc2.bias)
        return v1, v2, F.layer_norm(v2, (384,), d(layer.ln2.weight), d(layer.ln2.bias), layer.ln2.eps)

    with torch.no_grad():
        v1, v2, _ = reference()
        v = v1 if which == "ln1" else v2
        shift = ratio * float(v.std(1).mean())
        (layer.out.bias if which == "ln1" else layer.fc2.bias).add_(shift)
        v1, v2, ref = reference()
        v = v1 if which == "ln1" else v2
        measured = float((v.mean(1).abs() / v.std(1)).mean())
        got = fused_attn_out_mlp(a, res, layer)
    torch.cuda.synchronize()
    assert got is not None and not torch.isnan(got).any()
    return float((got.double().cpu() - ref).abs().max()), max(1.0, float(ref.abs().max())), measured


@pytest.mark.parametrize("which", ["ln1", "ln2"])
@pytest.mark.parametrize("ratio", [0, 2, 8, 32, 64, 120])
def test_layer_tail_one_pass_variance_on_rows_with_a_large_mean(ratio, which):
    """var = E[v^2] - mean^2 in fp32 loses about (mean / std)^2 x 2^-24 of the normalised value: up to mean / std = 32 (what the issue asks for; 64 and
    120 are run as well) that stays far inside the tolerance
    of tests/test_gpu_encoder_kernels.py::test_fused_attention_output_projection_and_mlp_h384 (1.2e-2 x scale), which is the one asserted here."""
    err, scale, measured = _variance_case(float(ratio), which)
    print(f"layer tail, {which} rows at mean/std {measured:.1f} (asked {ratio}): max|diff| vs fp64 {err:.3e}, scale {scale:.2f}, ratio {err / scale:.3e}", flush=True)
    assert measured >= 0.9 * ratio
    assert err <= 1.2e-2 * scale, (ratio, which, err, scale)
