"""A trained-shaped encoder and high-precision references for the composed-forward tests (tests/test_encoder_trained_like.py,
tests/test_gpu_encoder_trained_like.py, tests/emulated_encoder_cases.py).

``BertEncoder.random_init`` is normal(0, 0.02) weights, zero biases and identity LayerNorms: every softmax of such a model is almost
uniform, every FC1 pre-activation lies inside |x| < 1.5, and every bias / gamma / beta is interchangeable with every other one.
``trained_like_init`` overwrites it with parameters of the magnitudes a trained sentence encoder has -- sharp attention heads, GELU
inputs out to +-7, LayerNorm outliers -- all different from layer to layer, so that a swapped, shared or dropped parameter moves
the embeddings by far more than fp16 rounding does.

Everything here is plain torch / numpy on the CPU; the forward below is written out op by op (it does not call the encoder's own
forward), in the dtype of the parameters it is given: fp64 = the reference, fp16 = the level a well-behaved fp16 pipeline reaches."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from leann_amd.encoder import BertEncoder, EncoderConfig

LOG2E = 1.4426950408889634
QK_DEPTH_GAIN = 0.08
LAYER_TENSORS = ("qkv.weight", "qkv.bias", "out.weight", "out.bias", "ln1.weight", "ln1.bias", "fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias",
                 "ln2.weight", "ln2.bias")


def minilm_cfg(vocab: int = 2000, layers: int = 6, ffn: int = 1536, max_pos: int = 256, pooling: str = "mean") -> EncoderConfig:
    return EncoderConfig(vocab_size=vocab, hidden=384, layers=layers, heads=12, ffn=ffn, max_pos=max_pos, max_seq_length=max_pos, pooling=pooling)


def trained_like_init(cfg: EncoderConfig, seed: int = 0) -> BertEncoder:
    """fp32 weights on the CPU, seeded; no two parameter tensors alike, no zero bias, no unit gamma.  Standard deviations are those of the
    hidden-384 / ffn-1536 recipe, scaled by sqrt(reference fan-in / fan-in) for other widths so that the logits and the FC1 / FC2 outputs
    keep their spread (the attention logits' spread is the product of the Q and K spreads whatever head_dim is)."""
    enc = BertEncoder.random_init(cfg, seed)
    g = torch.Generator(device="cpu").manual_seed(7919 * seed + 104729)
    H, ffn = cfg.hidden, cfg.ffn
    s_h, s_f = math.sqrt(384.0 / H), math.sqrt(1536.0 / ffn)

    def N(*shape):
        return torch.randn(shape, generator=g)

    with torch.no_grad():
        enc.word.weight.copy_(0.05 * N(cfg.vocab_size, H))
        enc.pos.weight.copy_(0.02 * N(cfg.max_pos, H))
        enc.tok_type.weight.copy_(0.02 * N(cfg.type_vocab, H))
        enc.ln.weight.copy_(1.0 + 0.2 * N(H))
        enc.ln.bias.copy_(0.1 * N(H))
        for li, L in enumerate(enc.layers):
            qk = 0.11 * (1.0 + QK_DEPTH_GAIN * li)  # deeper layers see more alike rows: their Q / K grow to keep some heads sharp
            rows = torch.tensor([qk] * (2 * H) + [0.05] * H)[:, None] * s_h
            L.qkv.weight.copy_(N(3 * H, H) * rows)
            L.qkv.bias.copy_(0.3 * N(3 * H))
            L.out.weight.copy_(0.05 * s_h * N(H, H))
            L.out.bias.copy_(0.2 * N(H))
            L.fc1.weight.copy_(0.07 * s_h * N(ffn, H))
            L.fc1.bias.copy_(0.5 * N(ffn) - 0.3)
            L.fc2.weight.copy_(0.04 * s_f * N(H, ffn))
            L.fc2.bias.copy_(0.2 * N(H))
            L.fc1.bias[(53 * li + 17) % ffn] = 2.5  # one hidden unit per layer that is always on (the largest |bias| of the layer)
            for k, ln in enumerate((L.ln1, L.ln2)):
                ln.weight.copy_(0.9 + 0.25 * N(H))
                ln.bias.copy_(0.15 * N(H))
                base = 37 * li + 151 * k  # three outliers per LayerNorm, somewhere else in every layer
                ln.weight[(base + 5) % H] = 0.03
                ln.weight[(base + 101) % H] = 3.0
                ln.bias[(base + 211) % H] = -1.5
        for p in enc.parameters():  # "no bias is zero and no gamma is one": nudge the measure-zero accidents away
            if p.dim() == 1:
                p[p == 0.0] = 1e-3
        for ln in [enc.ln] + [x for L in enc.layers for x in (L.ln1, L.ln2)]:
            ln.weight[ln.weight.half() == 1.0] = 1.002  # (also after the fp16 rounding of the GPU model)
    return enc.eval()


def make_batch(cfg: EncoderConfig, lengths, seed: int = 0):
    """Padded int32 ids [n, max(lengths)] of random tokens (1 .. vocab - 1; 0 pads) + int32 lengths."""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lengths, np.int32)
    ids = np.zeros((lens.shape[0], int(lens.max())), np.int32)
    for i, l in enumerate(lens):
        ids[i, :l] = rng.integers(1, cfg.vocab_size, int(l))
    return torch.from_numpy(ids), torch.from_numpy(lens)


def params_of(enc: BertEncoder, dtype=torch.float64) -> dict:
    """{state-dict name: CPU tensor in ``dtype``} -- what forward_ref computes from (a copy: mutate it freely)."""
    return {k: v.detach().to("cpu", dtype).clone() for k, v in enc.state_dict().items()}


def forward_ref(cfg: EncoderConfig, P: dict, ids: torch.Tensor, lens: torch.Tensor, taps: dict = None, layer_of=None) -> torch.Tensor:
    """The BERT forward + pooling, sequence by sequence, in plain torch ops in the dtype of ``P``; pooled in fp64.  ``taps`` (a dict) receives,
    per layer, the attention logits in log2 units, the FC1 pre-activations and the layer outputs of every sequence.  ``layer_of(name, li)``
    names the layer whose tensor ``name`` layer ``li`` uses (wiring mutants); default: its own."""
    dt = P["word.weight"].dtype
    H, nh = cfg.hidden, cfg.heads
    hd = H // nh

    def p(li, name):
        return P[f"layers.{li if layer_of is None else layer_of(name, li)}.{name}"]

    out = torch.empty((ids.shape[0], H), dtype=torch.float64)
    for i in range(ids.shape[0]):
        n = int(lens[i])
        tok = ids[i, :n].long()
        x = P["word.weight"][tok] + P["pos.weight"][:n] + P["tok_type.weight"][0][None]
        x = F.layer_norm(x, (H,), P["ln.weight"], P["ln.bias"], cfg.ln_eps)
        for li in range(cfg.layers):
            qkv = F.linear(x, p(li, "qkv.weight"), p(li, "qkv.bias")).view(n, 3, nh, hd)
            q, k, v = (qkv[:, j].transpose(0, 1) for j in range(3))  # [heads, n, hd]
            sc = (q @ k.transpose(1, 2)) / math.sqrt(hd)
            a = (torch.softmax(sc, dim=-1) @ v).transpose(0, 1).reshape(n, H)
            x = F.layer_norm(x + F.linear(a, p(li, "out.weight"), p(li, "out.bias")), (H,), p(li, "ln1.weight"), p(li, "ln1.bias"), cfg.ln_eps)
            pre = F.linear(x, p(li, "fc1.weight"), p(li, "fc1.bias"))
            x = F.layer_norm(x + F.linear(F.gelu(pre), p(li, "fc2.weight"), p(li, "fc2.bias")), (H,), p(li, "ln2.weight"), p(li, "ln2.bias"), cfg.ln_eps)
            if taps is not None:
                t = taps.setdefault(li, {"log2_scores": [], "fc1_pre": [], "out": []})
                t["log2_scores"].append(sc.double() * LOG2E)
                t["fc1_pre"].append(pre.double())
                t["out"].append(x.double())
        xd = x.double()
        out[i] = xd[0] if cfg.pooling == "cls" else xd.mean(0)
    return F.normalize(out, p=2, dim=1) if cfg.normalize else out


@torch.no_grad()
def reference_fp64(enc: BertEncoder, ids: torch.Tensor, lens: torch.Tensor, taps: dict = None) -> torch.Tensor:
    """fp64 embeddings [n, hidden] of ``enc``'s CURRENT weights (wherever they live, whatever their dtype: the values are taken as they are)."""
    return forward_ref(enc.cfg, params_of(enc), ids.cpu(), lens.cpu(), taps)


@torch.no_grad()
def plain_fp16(enc: BertEncoder, ids: torch.Tensor, lens: torch.Tensor) -> torch.Tensor:
    """The same ops with fp16 parameters and activations in plain torch on the CPU: the error level of a straightforward fp16 pipeline."""
    return forward_ref(enc.cfg, params_of(enc, torch.float16), ids.cpu(), lens.cpu())


@torch.no_grad()
def describe(enc: BertEncoder, ids: torch.Tensor, lens: torch.Tensor) -> list:
    """Per layer, from the fp64 reference: ``sharp`` = share of (sequence, head, query) rows whose largest softmax weight exceeds 0.5; ``grew`` =
    rows whose maximum logit over keys 32.. exceeds the maximum over keys 0..31 by more than 8 log2 units (what forces the attention kernels'
    deferred-rescale branch); ``fc1_below`` / ``fc1_above`` = shares of FC1 pre-activations below -3 / above +3; ``fc1_min`` / ``fc1_max``."""
    taps = {}
    reference_fp64(enc, ids, lens, taps)
    rows = []
    for li in range(enc.cfg.layers):
        sharp = total = grew = 0
        for s2 in taps[li]["log2_scores"]:
            pm = torch.softmax(s2 / LOG2E, dim=-1).max(-1).values
            sharp += int((pm > 0.5).sum())
            total += pm.numel()
            if s2.shape[-1] > 32:
                grew += int(((s2[:, :, 32:].max(-1).values - s2[:, :, :32].max(-1).values) > 8.0).sum())
        pre = torch.cat([t.reshape(-1) for t in taps[li]["fc1_pre"]])
        rows.append({"sharp": sharp / total, "grew": grew, "fc1_below": float((pre < -3).double().mean()), "fc1_above": float((pre > 3).double().mean()),
                     "fc1_min": float(pre.min()), "fc1_max": float(pre.max())})
    return rows


# ---- the three wiring mutants of the reference (what a mis-filled parameter struct would compute) ---------------------------------------
def _swap_out_bias_with_fc2_bias(P, cfg):
    P["layers.3.out.bias"], P["layers.3.fc2.bias"] = P["layers.3.fc2.bias"], P["layers.3.out.bias"]
    return None


def _layer4_ln2_bias_in_layer5(P, cfg):
    return lambda name, li: 4 if (name == "ln2.bias" and li == 5) else li


def typical_element(b: torch.Tensor) -> int:
    """Index of the element of median magnitude (ties: the lower index)."""
    a = b.detach().double().cpu().abs()
    return int(torch.argsort(a, stable=True)[a.numel() // 2])


def _one_fc1_bias_element_zeroed(P, cfg):
    b = P["layers.2.fc1.bias"]
    b[typical_element(b)] = 0.0  # an ordinary element (0.5 N - 0.3 has median magnitude ~0.4): what one dropped bias load does
    return None


def _always_on_fc1_bias_zeroed(P, cfg):
    b = P["layers.2.fc1.bias"]
    b[int(b.abs().argmax())] = 0.0  # the 2.5 the init plants: a deliberately LOUD variant of the mutant above, not a typical element
    return None


MUTANTS = {"out.bias <-> fc2.bias in layer 3": _swap_out_bias_with_fc2_bias, "layer 4's ln2.bias used in layer 5": _layer4_ln2_bias_in_layer5,
           "one element of layer 2's fc1.bias zeroed": _one_fc1_bias_element_zeroed,
           "the always-on unit's fc1.bias of layer 2 zeroed": _always_on_fc1_bias_zeroed}


@torch.no_grad()
def mutant_fp64(enc: BertEncoder, ids: torch.Tensor, lens: torch.Tensor, name: str) -> torch.Tensor:
    P = params_of(enc)
    layer_of = MUTANTS[name](P, enc.cfg)
    return forward_ref(enc.cfg, P, ids.cpu(), lens.cpu(), None, layer_of)


def errors(got: torch.Tensor, ref: torch.Tensor) -> tuple:
    """(max |got - ref|, min cosine) against an fp64 reference."""
    g = got.detach().cpu().double()
    return float((g - ref).abs().max()), float(F.cosine_similarity(g, ref).min())


# ---- GELU -----------------------------------------------------------------------------------------------------------------------------
GELU_COEFFS = (-0.0004881171917077154, 0.007198805455118418, -0.052146803587675095, -0.4595957100391388, -1.1510006189346313)


def all_finite_fp16() -> np.ndarray:
    """Every finite fp16 value (63 488 of them: both zeros, the subnormals, up to +-65504), in bit-pattern order."""
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    v = bits.view(np.float16)
    return v[np.isfinite(v)]


def gelu_fp64(x) -> np.ndarray:
    """x Phi(x) = x erfc(-x / sqrt 2) / 2 in fp64 (math.erfc keeps the left tail's relative precision)."""
    x = np.asarray(x, np.float64)
    return np.array([0.5 * t * math.erfc(-t / math.sqrt(2.0)) for t in x.ravel()]).reshape(x.shape)


def gelu_poly_fp32(x) -> np.ndarray:
    """The kernels' GELU restated in numpy (csrc/lm_gemm_f16.hip: gm_gelu; csrc/lm_layer_tail_h384.hip: t4_gelu_uop), fp32 in, fp32 out:
    gelu(x) = max(x, 0) - u 2^(-1 - u q(u)), u = |x|, q a degree-4 polynomial, every step one fp32 fused multiply-add (product and sum in fp64 --
    the product of two fp32 is exact there -- rounded to fp32 once) and one exp2."""
    x = np.asarray(x, np.float32)
    u = np.abs(x).astype(np.float64)
    c = [np.float64(np.float32(v)) for v in GELU_COEFFS]

    def fma(a, b, d):
        with np.errstate(over="ignore"):
            return (a * b + d).astype(np.float32).astype(np.float64)

    p = fma(u, c[0], c[1])
    for k in (2, 3, 4):
        p = fma(p, u, c[k])
    with np.errstate(under="ignore"):
        w = np.exp2(fma(p, u, -1.0)).astype(np.float32).astype(np.float64)
    return fma(-u, w, np.maximum(x, np.float32(0)).astype(np.float64)).astype(np.float32)


def ulp16(v) -> np.ndarray:
    """Spacing of the fp16 grid at the fp64 value(s) v: 2^(floor(log2 |v|) - 10), 2^-24 in the subnormal range."""
    a = np.abs(np.asarray(v, np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -14)))
    return np.exp2(np.clip(e, -14, 15) - 10)


def gelu_sweep_report(x16: np.ndarray, got) -> dict:
    """Figures of a GELU over fp16 inputs ``x16`` (``got``: fp16 or fp32 results) against x Phi(x) in fp64: ``abs`` = max |got - ref|, ``excess`` = max of
    |got - ref| - (1e-6 + ulp16(ref) / 2) (<= 0: inside the kernels' stated fp32 bound + correct fp16 rounding), ``ulps_right`` = max |got - ref| /
    ulp16(ref) over x > -3, ``finite``, ``identity`` = got == x for x >= 6, ``zero`` = got == +-0 for x < -9."""
    x = x16.astype(np.float64)
    ref = gelu_fp64(x)
    g = np.asarray(got).astype(np.float64)
    finite = bool(np.isfinite(g).all())
    d = np.abs(np.where(np.isfinite(g), g, 0.0) - ref)
    right = x > -3.0
    return {"abs": float(d.max()), "excess": float((d - (1e-6 + 0.5 * ulp16(ref))).max()), "ulps_right": float((d[right] / ulp16(ref[right])).max()),
            "finite": finite, "identity": bool((g[x >= 6.0] == x[x >= 6.0]).all()), "zero": bool((g[x < -9.0] == 0.0).all())}


def assert_gelu_sweep(rep: dict) -> None:
    assert rep["finite"], rep
    assert rep["excess"] <= 0.0, rep      # |got - ref| <= 1e-6 + half an fp16 ulp of ref
    assert rep["ulps_right"] <= 1.0, rep  # x > -3: at most one fp16 ulp
    assert rep["identity"] and rep["zero"], rep


def tail_gelu_sweep() -> np.ndarray:
    """1536 fp16-representable FC1 biases for the layer-tail GELU sweep, 4 x 384 (launch s routes units 384 s .. 384 s + 383): launches 0 .. 2 a dense grid
    on [-9.5, 9.5] (interleaved, so that every launch's row spans the whole interval and its LayerNorm has the same spread), launch 3 a coarser grid + the
    extremes (+-65504, +-2^-14, +-2^-24, +-0, +-1000, the kernel's corner values) -- kept in one launch because one 65504 in a row flattens everything
    else in that row's LayerNorm."""
    grid = np.linspace(-9.5, 9.5, 1152).astype(np.float16)
    special = np.array([65504, -65504, 2.0 ** -14, -(2.0 ** -14), 2.0 ** -24, -(2.0 ** -24), 0.0, -0.0, 1000, -1000, 6.0, -9.0, -3.0, 9.5, -9.5, 11.0, -11.0,
                        60.0, -60.0, 1.0, -1.0, 0.5, -0.5], np.float16)
    coarse = np.linspace(-9.5, 9.5, 384 - special.shape[0]).astype(np.float16)
    out = np.empty(1536, np.float16)
    for s in range(3):
        out[384 * s: 384 * (s + 1)] = grid[s::3]
    out[1152:] = np.concatenate([special, coarse])
    return out


def tail_gelu_reference(b1_row: np.ndarray, eps: float = 1e-12) -> tuple:
    """(reference, bound) of one launch of the layer-tail GELU sweep: the row is v_c = fp16(gelu(b1_c)), the output its LayerNorm (gamma 1, beta 0).
    Bound = (a) what the GELU bound of the sweep above (|g - t| <= 1e-6 + half an fp16 ulp of the unrounded t) allows the kernel's fp16 value g to differ
    from the correctly rounded v: nothing, unless t lies within 1e-6 of the midpoint of two fp16 neighbours -- then D_c = 1e-6 + ulp16(t_c) -- propagated
    to first order through y_c = (v_c - mu) rstd:
        |dy_c| <= rstd (D_c + mean D) + |v_c - mu| rstd^3 / n * sum_i |v_i - mu| (D_i + mean D),
    (b) the fp32 arithmetic of the one-pass LayerNorm: 2^-20 * E[v^2] / var relative on both terms of v rstd - mu rstd, (c) half an fp16 ulp of the
    output."""
    t = gelu_fp64(b1_row.astype(np.float64))
    v = t.astype(np.float16).astype(np.float64)
    n = v.shape[0]
    mu, var = v.mean(), v.var()
    rstd = 1.0 / math.sqrt(var + eps)
    y = (v - mu) * rstd
    u = ulp16(t)
    to_midpoint = np.abs(np.mod(t / u, 1.0) - 0.5) * u
    D = np.where(to_midpoint > 1e-6, 0.0, 1e-6 + u)
    dv = D + D.mean()
    prop = rstd * dv + np.abs(v - mu) * rstd ** 3 / n * float((np.abs(v - mu) * dv).sum())
    fp32 = 2.0 ** -20 * ((v * v).mean() / var) * (np.abs(v) * rstd + abs(mu) * rstd)
    return y, prop + fp32 + 0.5 * ulp16(y)
