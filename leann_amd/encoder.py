"""In-process sentence-embedding encoder (BERT family) on PyTorch-ROCm.

Replaces the embedding-recompute server of the reference for the search path:
``compute_embeddings_sentence_transformers`` (packages/leann-core/src/leann/embedding_compute.py:71-353:
fp16 on GPU :157-162,199-204, model.encode :229-239, manual mean-pool path :323-334) running
inside ``hnsw_embedding_server.py``.  Same arithmetic as sentence-transformers' Transformer ->
Pooling(mean|cls) -> optional Normalize stack; weights are loaded from a Hugging Face BERT
checkpoint when one is available locally, otherwise seeded random weights of the identical
architecture (throughput-identical; there is no network in the build/bench environment).

MFMA is used only here, and only inside hand-written kernels (csrc/): hidden 384 -- weight-stationary QKV GEMM, varlen attention,
fused attention-output + LayerNorm + feed-forward + LayerNorm; hidden 768 and small forwards -- the general GEMM lm_gemm_f16 with
bias / GELU / residual epilogues, the same attention kernel at head_dim 64, LayerNorm.  Library GEMMs (hipBLASLt) and torch's varlen
attention remain only as the A/B paths the LEANN_MI355X_* switches select and for shapes outside the kernels' envelopes (CPU, fp32).
"""

from __future__ import annotations

from dataclasses import dataclass, replace
from pathlib import Path
from typing import Optional

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F


@dataclass(frozen=True)
class EncoderConfig:
    vocab_size: int = 30522
    hidden: int = 384
    layers: int = 6
    heads: int = 12
    ffn: int = 1536
    max_pos: int = 512
    type_vocab: int = 2
    ln_eps: float = 1e-12
    pooling: str = "mean"  # "mean" | "cls"
    normalize: bool = True
    max_seq_length: int = 256
    pad_id: int = 0

    @property
    def dim(self) -> int:
        return self.hidden

    def flops_per_chunk(self, T: int) -> float:
        """2*P_enc*T + 4*L*T^2*H."""
        p_layer = 4 * self.hidden * self.hidden + 2 * self.hidden * self.ffn
        return 2.0 * self.layers * p_layer * T + 4.0 * self.layers * T * T * self.hidden


# architecture presets for the models BASELINE.json names
PRESETS = {
    "all-minilm-l6-v2": EncoderConfig(hidden=384, layers=6, heads=12, ffn=1536, pooling="mean", normalize=True, max_seq_length=256),
    "bge-small-en-v1.5": EncoderConfig(hidden=384, layers=12, heads=12, ffn=1536, pooling="cls", normalize=True, max_seq_length=512),
    "bge-base-en-v1.5": EncoderConfig(hidden=768, layers=12, heads=12, ffn=3072, pooling="cls", normalize=True, max_seq_length=512),
    "contriever": EncoderConfig(hidden=768, layers=12, heads=12, ffn=3072, pooling="mean", normalize=False, max_seq_length=512),
    "all-mpnet-base-v2": EncoderConfig(hidden=768, layers=12, heads=12, ffn=3072, pooling="mean", normalize=True, max_seq_length=384),
}


def config_for(model_name: str, strict: bool = False) -> EncoderConfig:
    """Architecture preset by model name.  ``strict`` (every path that loads REAL weights) raises for a name that
    matches no preset instead of assuming the MiniLM one: a wrong pooling / normalisation / length cap would
    silently produce embeddings unrelated to the ones the index was built from."""
    key = (model_name or "").lower()
    for k, v in PRESETS.items():
        if k in key:
            return v
    if strict:
        raise ValueError(f"no architecture preset for embedding model {model_name!r}; known: {sorted(PRESETS)}")
    return PRESETS["all-minilm-l6-v2"]


def _read_json(path: Path) -> Optional[dict]:
    import json

    try:
        with open(path, encoding="utf-8") as f:
            return json.load(f)
    except (OSError, ValueError):
        return None


def sentence_transformers_settings(model_dir: Path) -> dict:
    """Pooling / normalisation / max_seq_length as the checkpoint's own sentence-transformers files state them
    (modules.json, 1_Pooling/config.json, sentence_bert_config.json) -- what ``SentenceTransformer(...).encode``
    applies in the reference (embedding_compute.py:229-239 passes normalize_embeddings=False, so normalisation is
    exactly the presence of a Normalize module).  Keys absent from the result were not stated by the checkpoint."""
    out: dict = {}
    mods = _read_json(model_dir / "modules.json")
    if isinstance(mods, list):
        types = [str(m.get("type", "")) for m in mods]
        out["normalize"] = any(t.endswith("Normalize") for t in types)
        for m in mods:
            if str(m.get("type", "")).endswith("Pooling"):
                pc = _read_json(model_dir / m.get("path", "1_Pooling") / "config.json") or {}
                if pc.get("pooling_mode_cls_token"):
                    out["pooling"] = "cls"
                elif pc.get("pooling_mode_mean_tokens"):
                    out["pooling"] = "mean"
                elif pc:
                    raise ValueError(f"unsupported sentence-transformers pooling in {model_dir}: {pc}")
    sb = _read_json(model_dir / "sentence_bert_config.json")
    if sb and sb.get("max_seq_length"):
        out["max_seq_length"] = int(sb["max_seq_length"])
    return out


class KernelTimers:
    """HIP-event pairs around the hand-written encoder kernels (on torch's current stream = the stream they are launched on).
    bench.py switches it on for its whole run -- ``KernelTimers.active = KernelTimers()`` -- and labels the phases
    (``.phase = "timed"``), so the dominant kernel's duration is measured live over the timed region AND over every launch of the
    process (the quantity a ``rocprofv3 --kernel-trace --stats`` table of the same command averages).  Cost: two event records
    per launch (~2 us against a ~700 us kernel).  Off (``active is None``) everywhere else."""

    active: "Optional[KernelTimers]" = None

    def __init__(self):
        self.pairs: dict = {}
        self.phase = "setup"

    def span(self, name: str, work: float):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.pairs.setdefault(name, []).append((a, b, work, self.phase))
        return a, b

    def totals(self, phase: Optional[str] = None) -> dict:
        """{kernel: {"ms", "work", "launches"}} over the launches of ``phase`` (None: every launch so far)."""
        torch.cuda.synchronize()
        out = {}
        for k, v in self.pairs.items():
            sel = [(a, b, w) for a, b, w, ph in v if phase is None or ph == phase]
            out[k] = {"ms": sum(a.elapsed_time(b) for a, b, _ in sel), "work": sum(w for _, _, w in sel), "launches": len(sel)}
        return out


def _src_key(*tensors: torch.Tensor) -> tuple:
    """Identity of the weights a packed copy was made from: device, storage address, in-place version counter and dtype of every
    source tensor.  ``load_state_dict`` / an optimiser step / ``.copy_`` bump ``_version``; ``.to(dtype=...)`` / ``.half()`` replace
    the storage -- either way the key changes and the pack is rebuilt instead of silently serving stale or wrong-dtype weights."""
    return tuple((t.device, t.data_ptr(), t._version, t.dtype) for t in tensors)


def _packed(owner, attr: str, sources: tuple, make):
    """``owner.<attr>`` = (key, pack) cache of ``make()`` keyed on ``_src_key(*sources)``."""
    key = _src_key(*sources)
    ent = getattr(owner, attr, None)
    if ent is None or ent[0] != key:
        ent = (key, make())
        setattr(owner, attr, ent)
    return ent[1]


# environment variables that select a particular kernel generation for an A/B run (everything else under LEANN_MI355X_* --
# ALLOW_RANDOM_WEIGHTS, ATTN_XCD, STAGGER ... -- does not change which kernels a forward is made of)
KERNEL_SELECTION_KEYS = ("LEANN_MI355X_QKV", "LEANN_MI355X_ATTN", "LEANN_MI355X_LN", "LEANN_MI355X_POOL", "LEANN_MI355X_EMBED", "LEANN_MI355X_PACK",
                         "LEANN_MI355X_LINEAR", "LEANN_MI355X_TAIL", "LEANN_MI355X_TAIL4", "LEANN_MI355X_GEMM")


def fused_add_layernorm(x: torch.Tensor, residual: Optional[torch.Tensor], ln: nn.LayerNorm) -> torch.Tensor:
    """LayerNorm(x + residual) through the hand-written HIP kernel (csrc/lm_encoder_ops2.hip, 16 lanes per row) for fp16 CUDA
    tensors; plain torch otherwise (CPU / fp32 parity paths)."""
    if x.is_cuda and x.dtype == torch.float16 and x.shape[-1] % 8 == 0 and x.is_contiguous() and (
            residual is None or residual.is_contiguous()):
        import ctypes as C

        from . import _lib

        out = torch.empty_like(x)
        rows = x.numel() // x.shape[-1]
        _lib.check(_lib.load().lm_add_layernorm_f16(
            C.c_void_p(x.data_ptr()), C.c_void_p(residual.data_ptr()) if residual is not None else None,
            C.c_void_p(ln.weight.data_ptr()), C.c_void_p(ln.bias.data_ptr()), C.c_void_p(out.data_ptr()), rows,
            x.shape[-1], float(ln.eps), C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)), "lm_add_layernorm_f16")
        return out
    return ln(x if residual is None else x + residual)


def fused_attention_hd32(qkv: torch.Tensor, cu: torch.Tensor, heads: int, max_len: int) -> Optional[torch.Tensor]:
    """Hand-written MFMA varlen attention (csrc/lm_attn_v3.hip, lm_attn_v2.hip) for head_dim 32 and 64, lengths <= 512, fp16 on the
    GPU; returns None when the shape is outside that envelope (caller falls back to torch's varlen_attn)."""
    import os

    tot, h3 = qkv.shape
    hidden = h3 // 3
    hd = hidden // heads if heads else 0
    if not (qkv.is_cuda and qkv.dtype == torch.float16 and qkv.is_contiguous() and hidden == heads * hd
            and hd in (32, 64) and 0 < max_len <= 512):
        return None
    if os.environ.get("LEANN_MI355X_ATTN", "1") == "0":  # torch's varlen_attn (A/B)
        return None
    import ctypes as C

    from . import _lib

    out = torch.empty((tot, hidden), dtype=torch.float16, device=qkv.device)
    st = C.c_void_p(torch.cuda.current_stream(qkv.device).cuda_stream)
    if hd == 32:
        _lib.check(_lib.load().lm_attn_varlen_hd32_f16(C.c_void_p(qkv.data_ptr()), C.c_void_p(cu.data_ptr()), cu.shape[0] - 1, heads, int(max_len),
                                                       C.c_void_p(out.data_ptr()), st), "lm_attn_varlen_hd32_f16")
    else:
        _lib.check(_lib.load().lm_attn_varlen_f16(C.c_void_p(qkv.data_ptr()), C.c_void_p(cu.data_ptr()), cu.shape[0] - 1, heads, hd, int(max_len),
                                                  C.c_void_p(out.data_ptr()), st), "lm_attn_varlen_f16")
    return out


GEMM_EPI_GELU, GEMM_EPI_RESIDUAL = 1, 2
LM_BERT_SMALL_TOKENS = 8192  # include/leann_mi355x.h


def small_tokens_limit() -> int:
    """Forwards of at most this many tokens run the hidden-384 layers on the general kernels (LEANN_MI355X_SMALL_TOKENS overrides; 0 = never)."""
    import os

    return int(os.environ.get("LEANN_MI355X_SMALL_TOKENS", LM_BERT_SMALL_TOKENS))


LM_BERT_QKV_GEMM_TOKENS = 45056  # include/leann_mi355x.h


def qkv_gemm_tokens_limit() -> int:
    """A LARGE-form hidden-384 forward of at most this many tokens takes its QKV projection from the general GEMM (round 6: the streaming kernel's
    256-token workgroup is a ~45 us chain however few CUs the forward fills; include/leann_mi355x.h: LM_BERT_QKV_GEMM_TOKENS).  Mirrors
    csrc/lm_encoder_forward.cpp: LEANN_MI355X_QKV_GEMM_TOKENS overrides, LEANN_MI355X_SMALL_TOKENS=0 ("the large-forward kernels at every size") implies 0."""
    import os

    if "LEANN_MI355X_QKV_GEMM_TOKENS" in os.environ:
        return int(os.environ["LEANN_MI355X_QKV_GEMM_TOKENS"])
    if os.environ.get("LEANN_MI355X_SMALL_TOKENS") is not None and int(os.environ["LEANN_MI355X_SMALL_TOKENS"]) == 0:
        return 0
    return LM_BERT_QKV_GEMM_TOKENS


def fused_gemm(x: torch.Tensor, lin: nn.Linear, epilogue: int = 0, residual: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """epi(x W^T + b) through the general hand-written MFMA GEMM (csrc/lm_gemm_f16.hip: 256 x 256 tiles, operands staged L2 -> LDS by
    DMA, bias / exact-erf GELU / residual in the epilogue): the linear layers of every model whose hidden size is not 384 (bge-base,
    contriever: 768).  ``epilogue`` = GEMM_EPI_GELU | GEMM_EPI_RESIDUAL.  LEANN_MI355X_GEMM=0 = library GEMMs (A/B); None = not
    applicable, the caller takes the library path."""
    import os

    if os.environ.get("LEANN_MI355X_GEMM", "1") == "0":
        return None
    n, k = lin.weight.shape
    if not (x.is_cuda and x.dtype == torch.float16 and x.is_contiguous() and lin.weight.dtype == torch.float16 and n % 128 == 0 and k % 128 == 0
            and lin.bias is not None and x.shape[-1] == k):
        return None
    if (epilogue & GEMM_EPI_RESIDUAL) and not (residual is not None and residual.is_contiguous() and residual.dtype == torch.float16
                                               and tuple(residual.shape) == (x.shape[0], n)):
        return None
    import ctypes as C

    from . import _lib

    w, b = _packed(lin, "_gemm_pack", (lin.weight, lin.bias), lambda: (lin.weight.detach().contiguous(), lin.bias.detach().float().contiguous()))
    out = torch.empty((x.shape[0], n), dtype=torch.float16, device=x.device)
    tm = KernelTimers.active
    ev = tm.span("gemm_f16", 2.0 * x.shape[0] * n * k) if tm is not None else None
    if ev:
        ev[0].record()
    _lib.check(_lib.load().lm_gemm_f16(C.c_void_p(x.data_ptr()), C.c_void_p(w.data_ptr()), C.c_void_p(b.data_ptr()),
                                       C.c_void_p(residual.data_ptr()) if residual is not None else None, int(epilogue), n, k,
                                       C.c_void_p(out.data_ptr()), x.shape[0], C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)),
               "lm_gemm_f16")
    if ev:
        ev[1].record()
    return out


def fused_embed_layernorm(tok: torch.Tensor, pos: torch.Tensor, word: nn.Embedding, posw: nn.Embedding, type0: torch.Tensor,
                          ln: nn.LayerNorm) -> Optional[torch.Tensor]:
    """Embedding gathers + adds + LayerNorm in one kernel (csrc/lm_encoder_ops2.hip).  Default on (LEANN_MI355X_EMBED=0 = torch path, A/B); None = not applicable, the caller takes the torch path."""
    import os

    if os.environ.get("LEANN_MI355X_EMBED", "1") != "1":
        return None
    h = word.weight.shape[1]
    if not (tok.is_cuda and word.weight.dtype == torch.float16 and h % 8 == 0 and h <= 768):
        return None
    import ctypes as C

    from . import _lib

    t32, p32 = tok.to(torch.int32).contiguous(), pos.to(torch.int32).contiguous()
    out = torch.empty((t32.shape[0], h), dtype=torch.float16, device=tok.device)
    _lib.check(_lib.load().lm_embed_layernorm_f16(
        C.c_void_p(t32.data_ptr()), C.c_void_p(p32.data_ptr()), C.c_void_p(word.weight.data_ptr()), C.c_void_p(posw.weight.data_ptr()),
        C.c_void_p(type0.contiguous().data_ptr()), C.c_void_p(ln.weight.data_ptr()), C.c_void_p(ln.bias.data_ptr()),
        C.c_void_p(out.data_ptr()), t32.shape[0], h, float(ln.eps), C.c_void_p(torch.cuda.current_stream(tok.device).cuda_stream)),
        "lm_embed_layernorm_f16")
    return out


def fused_pack_tokens(ids: torch.Tensor, lens: torch.Tensor, cu: torch.Tensor, total: int):
    """Padded ids [n, t] + lengths + cumulative lengths -> (packed token ids, positions), int32 [total], in one kernel
    (csrc/lm_encoder_ops2.hip) instead of three boolean-mask selects.  Default on (LEANN_MI355X_PACK=0 = torch path, A/B); None = the caller takes the torch path."""
    import os

    if os.environ.get("LEANN_MI355X_PACK", "1") != "1":
        return None
    if not (ids.is_cuda and ids.dtype == torch.int32 and ids.is_contiguous() and lens.dtype == torch.int32 and cu.dtype == torch.int32):
        return None
    import ctypes as C

    from . import _lib

    n, t = ids.shape
    tok = torch.empty((total,), dtype=torch.int32, device=ids.device)
    pos = torch.empty((total,), dtype=torch.int32, device=ids.device)
    _lib.check(_lib.load().lm_pack_tokens(
        C.c_void_p(ids.data_ptr()), C.c_void_p(lens.contiguous().data_ptr()), C.c_void_p(cu.data_ptr()), n, t, C.c_void_p(tok.data_ptr()),
        C.c_void_p(pos.data_ptr()), C.c_void_p(torch.cuda.current_stream(ids.device).cuda_stream)), "lm_pack_tokens")
    return tok, pos


def fused_meanpool(x: torch.Tensor, cu: torch.Tensor, normalize: bool, cls: bool = False) -> Optional[torch.Tensor]:
    """Segmented mean -- or, with ``cls``, the first token -- (+ L2 normalise) over packed sequences (csrc/lm_encoder_ops2.hip), fp32 [n, H].
    Default on (LEANN_MI355X_POOL=0 = torch path, A/B); None = the caller takes the torch path."""
    import os

    if os.environ.get("LEANN_MI355X_POOL", "1") != "1":
        return None
    h = x.shape[1]
    if not (x.is_cuda and x.dtype == torch.float16 and x.is_contiguous() and h % 8 == 0 and h <= 2048):
        return None
    import ctypes as C

    from . import _lib

    n = cu.shape[0] - 1
    out = torch.empty((n, h), dtype=torch.float32, device=x.device)
    fn = _lib.load().lm_clspool_varlen_f16 if cls else _lib.load().lm_meanpool_varlen_f16
    _lib.check(fn(C.c_void_p(x.data_ptr()), C.c_void_p(cu.data_ptr()), n, h, 1 if normalize else 0, C.c_void_p(out.data_ptr()),
                  C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)), "lm_clspool_varlen_f16" if cls else "lm_meanpool_varlen_f16")
    return out


def fused_mlp_k_permutation() -> torch.Tensor:
    """Order of the 32 hidden units of a slab inside a packed W2 row (csrc/lm_layer_tail_h384.hip): position
    16u + 8g + e holds unit 16u + 4g + e (e < 4) or 16u + 8 + 4g + e - 4 (e >= 4) -- the hidden units whose GELU
    outputs lane group g already has in registers 8u .. 8u+7 of the first product's accumulator."""
    pos = torch.arange(32)
    u, g, e = pos // 16, (pos % 16) // 8, pos % 8
    return torch.where(e < 4, 16 * u + 4 * g + e, 16 * u + 8 + 4 * g + e - 4)


def pack_w2_fused_mlp(w2: torch.Tensor) -> torch.Tensor:
    """nn.Linear weight [H, F] -> [F/32, H, 32] slabs with the k permutation above (contiguous 24 KB per slab)."""
    h, f = w2.shape
    perm = fused_mlp_k_permutation().to(w2.device)
    return w2.reshape(h, f // 32, 32)[:, :, perm].permute(1, 0, 2).contiguous()


def pack_wo_slabs(wo: torch.Tensor) -> torch.Tensor:
    """nn.Linear weight [384, 384] of the attention output projection -> [12, 384, 32] slabs, NATURAL k order (slab s = input
    features 32 s .. 32 s + 31): the B operand of that product is the attention output as loaded from memory."""
    h, k = wo.shape
    return wo.reshape(h, k // 32, 32).permute(1, 0, 2).contiguous()


def pack_w1_acc_order(w1: torch.Tensor) -> torch.Tensor:
    """W1 [F, 384] with its columns in ACCUMULATOR order: column 32 j + p holds input feature 32 j + perm[p] (perm =
    fused_mlp_k_permutation).  csrc/lm_layer_tail_h384.hip: k_layer_tail_h384 normalises the attention block's output inside the
    MFMA accumulators and feeds those registers to the first product as they are."""
    f, h = w1.shape
    perm = fused_mlp_k_permutation().to(w1.device)
    return w1.reshape(f, h // 32, 32)[:, :, perm].reshape(f, h).contiguous()


def pack_tail_images(wo: torch.Tensor, w1: torch.Tensor, w2: torch.Tensor) -> tuple:
    """The three weight matrices of a layer tail as the LDS IMAGES csrc/lm_layer_tail_h384.hip streams (fp16, on the weights' device):
    pack_wo_slabs / pack_w1_acc_order / pack_w2_fused_mlp, then the library's own chunk swizzle (lm_layer_tail_pack_h384) -- one
    definition of the image layout, next to the kernel that reads it."""
    import ctypes as C

    from . import _lib

    if not (wo.is_cuda and w1.is_cuda and w2.is_cuda):  # lm_layer_tail_pack_h384 is a DEVICE kernel over these pointers
        raise ValueError("pack_tail_images: the weights must be on the GPU (the image is written by a device kernel)")
    wos, w1a, w2p = pack_wo_slabs(wo.detach()), pack_w1_acc_order(w1.detach()), pack_w2_fused_mlp(w2.detach())
    imgs = tuple(torch.empty_like(s) for s in (wos, w1a, w2p))
    st = C.c_void_p(torch.cuda.current_stream(wo.device).cuda_stream)
    _lib.check(_lib.load().lm_layer_tail_pack_h384(C.c_void_p(wos.data_ptr()), C.c_void_p(w1a.data_ptr()), C.c_void_p(w2p.data_ptr()), int(w1.shape[0]),
                                                   *(C.c_void_p(i.data_ptr()) for i in imgs), st), "lm_layer_tail_pack_h384")
    return imgs  # (the packed sources die with this frame: the kernels above run on the stream the caching allocator orders their reuse on)


def fused_attn_out_mlp(a: torch.Tensor, resid: torch.Tensor, layer: "_Layer") -> Optional[torch.Tensor]:
    """LayerNorm2(x + fc2(GELU(fc1(x)))) with x = LayerNorm1(resid + out(a)) in ONE kernel (csrc/lm_layer_tail_h384.hip:
    k_layer_tail_h384, generation 4 of the fused layer tail) for hidden 384, fp16 on the GPU, ffn a multiple of 192.
    LEANN_MI355X_TAIL=0 = the unfused path (weight-stationary out-projection + LayerNorm, then the general GEMM for the feed-forward
    block: A/B); None = the caller takes that path."""
    import os

    if os.environ.get("LEANN_MI355X_TAIL", "1") != "1" or os.environ.get("LEANN_MI355X_LINEAR", "1") == "0":
        return None
    f, h = layer.fc1.weight.shape
    if not (a.is_cuda and a.dtype == torch.float16 and a.is_contiguous() and resid.is_contiguous() and resid.dtype == torch.float16
            and h == 384 and f % 192 == 0 and 192 <= f <= 1728 and layer.out.bias is not None):
        return None
    import ctypes as C

    from . import _lib

    wo_i, bo, w1_i, b1, w2_i, b2 = _packed(
        layer, "_tail_pack", (layer.out.weight, layer.out.bias, layer.fc1.weight, layer.fc1.bias, layer.fc2.weight, layer.fc2.bias),
        lambda: (lambda im: (im[0], layer.out.bias.detach().float().contiguous(), im[1], layer.fc1.bias.detach().float().contiguous(), im[2],
                             layer.fc2.bias.detach().float().contiguous()))(pack_tail_images(layer.out.weight, layer.fc1.weight, layer.fc2.weight)))
    out = torch.empty_like(resid)
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    tm = KernelTimers.active
    ev = tm.span("layer_tail_h384", a.shape[0] * (4.0 * f * h + 2.0 * h * h)) if tm is not None else None
    if ev:
        ev[0].record()
    _lib.check(_lib.load().lm_layer_tail_h384_f16(
        vp(a), vp(resid), vp(wo_i), vp(bo), vp(layer.ln1.weight), vp(layer.ln1.bias), float(layer.ln1.eps), vp(w1_i), vp(b1), vp(w2_i), vp(b2),
        vp(layer.ln2.weight), vp(layer.ln2.bias), vp(out), a.shape[0], f, float(layer.ln2.eps),
        C.c_void_p(torch.cuda.current_stream(a.device).cuda_stream)), "lm_layer_tail_h384_f16")
    if ev:
        ev[1].record()
    return out


def fused_linear_h384(x: torch.Tensor, lin: nn.Linear, residual: Optional[torch.Tensor] = None,
                      ln: Optional[nn.LayerNorm] = None) -> Optional[torch.Tensor]:
    """x W^T + b (and, with residual + ln, LayerNorm(residual + x W^T + b)) for 384 input features through the hand-written MFMA
    kernels: the weight-streaming QKV kernel (csrc/lm_qkv_h384.hip) or the weight-stationary GEMM (csrc/lm_gemm_ws_h384.hip, + the
    add+LayerNorm kernel for the output projection).  LEANN_MI355X_LINEAR=0 = the library path (A/B).  None = the caller takes the
    hipBLASLt path."""
    import os

    if os.environ.get("LEANN_MI355X_LINEAR", "1") == "0":
        return None
    return _linear_ws_h384(x, lin, residual, ln)


def pack_qkv_image(w: torch.Tensor) -> torch.Tensor:
    """nn.Linear weight [n_out, 384] -> the LDS image csrc/lm_qkv_h384.hip streams (lm_qkv_pack_h384; same size, on the weight's device)."""
    import ctypes as C

    from . import _lib

    if not w.is_cuda:  # lm_qkv_pack_h384 is a DEVICE kernel over these pointers
        raise ValueError("pack_qkv_image: the weight must be on the GPU (the image is written by a device kernel)")
    src = w.detach().contiguous()
    img = torch.empty_like(src)
    st = C.c_void_p(torch.cuda.current_stream(w.device).cuda_stream)
    _lib.check(_lib.load().lm_qkv_pack_h384(C.c_void_p(src.data_ptr()), int(src.shape[0]), C.c_void_p(img.data_ptr()), st), "lm_qkv_pack_h384")
    return img


def fused_qkv_attention(x: torch.Tensor, lin: nn.Linear, cu: torch.Tensor, heads: int, max_len: int, force: bool = False) -> Optional[torch.Tensor]:
    """softmax(Q K^T / sqrt(32)) V per (sequence, head) with [Q | K | V] = x W^T + b computed inside the kernel (csrc/lm_qkv_attn_h384.hip, round 6:
    the projection's 604 MB per 262 k tokens never go to HBM) -- the first half of a LARGE hidden-384 layer on forwards of long sequences.  None = the
    caller takes the stand-alone pair: another shape, or the library's own decision says so (lm_h384_first_half_form: mean sequence length below 216,
    LEANN_MI355X_FUSED_QKV_ATTN=0, the switches of the older attention generations; the one-call forward asks the same function, so both launch
    paths run the same kernels).  ``force`` (kernel tests): launch it whatever the decision would be."""
    import ctypes as C

    from . import _lib

    n, k = lin.weight.shape
    if not (x.is_cuda and x.dtype == torch.float16 and x.is_contiguous() and k == 384 and n == 1152 and heads == 12 and lin.bias is not None
            and 0 < max_len <= 256 and cu.dtype == torch.int32):
        return None
    lib = _lib.load()
    if not force and lib.lm_h384_first_half_form(int(heads), int(max_len), int(x.shape[0]), int(cu.shape[0] - 1)) != 0:
        return None
    pk = _packed(lin, "_qkv_pack", (lin.weight, lin.bias), lambda: (pack_qkv_image(lin.weight), lin.bias.detach().float().contiguous()))
    out = torch.empty((x.shape[0], 384), dtype=torch.float16, device=x.device)
    tm = KernelTimers.active
    ev = tm.span("qkv_attn_h384", x.shape[0] * 2.0 * 384 * 1152) if tm is not None else None
    if ev:
        ev[0].record()
    _lib.check(lib.lm_qkv_attn_h384_f16(C.c_void_p(x.data_ptr()), C.c_void_p(pk[0].data_ptr()), C.c_void_p(pk[1].data_ptr()), C.c_void_p(cu.data_ptr()),
                                        int(cu.shape[0] - 1), int(max_len), int(x.shape[0]), C.c_void_p(out.data_ptr()),
                                        C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)), "lm_qkv_attn_h384_f16")
    if ev:
        ev[1].record()
    return out


def _linear_ws_h384(x: torch.Tensor, lin: nn.Linear, residual: Optional[torch.Tensor], ln: Optional[nn.LayerNorm]) -> Optional[torch.Tensor]:
    n, k = lin.weight.shape
    if not (x.is_cuda and x.dtype == torch.float16 and x.is_contiguous() and k == 384 and n % 192 == 0 and n <= 6144 and lin.bias is not None):
        return None
    import ctypes as C
    import os

    from . import _lib

    if ln is None and n % 128 == 0 and n >= 256 and os.environ.get("LEANN_MI355X_QKV", "1") == "1":
        # the weight-STREAMING form (csrc/lm_qkv_h384.hip: x read once, two waves per SIMD); LEANN_MI355X_QKV=0 = the weight-stationary kernel (A/B)
        pk = _packed(lin, "_qkv_pack", (lin.weight, lin.bias), lambda: (pack_qkv_image(lin.weight), lin.bias.detach().float().contiguous()))
        out = torch.empty((x.shape[0], n), dtype=torch.float16, device=x.device)
        _lib.check(_lib.load().lm_qkv_h384_f16(C.c_void_p(x.data_ptr()), C.c_void_p(pk[0].data_ptr()), C.c_void_p(pk[1].data_ptr()), n,
                                               C.c_void_p(out.data_ptr()), x.shape[0], C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)),
                   "lm_qkv_h384_f16")
        return out

    pk = _packed(lin, "_ws_pack", (lin.weight, lin.bias), lambda: (lin.weight.detach().contiguous(), lin.bias.detach().float().contiguous()))
    out = torch.empty((x.shape[0], n), dtype=torch.float16, device=x.device)
    _lib.check(_lib.load().lm_gemm_ws_h384_f16(C.c_void_p(x.data_ptr()), C.c_void_p(pk[0].data_ptr()), C.c_void_p(pk[1].data_ptr()), n,
                                               C.c_void_p(out.data_ptr()), x.shape[0], C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)),
               "lm_gemm_ws_h384_f16")
    if ln is None:
        return out
    return fused_add_layernorm(out, residual, ln)


class _Layer(nn.Module):
    def __init__(self, c: EncoderConfig):
        super().__init__()
        self.qkv = nn.Linear(c.hidden, 3 * c.hidden)
        self.out = nn.Linear(c.hidden, c.hidden)
        self.ln1 = nn.LayerNorm(c.hidden, eps=c.ln_eps)
        self.fc1 = nn.Linear(c.hidden, c.ffn)
        self.fc2 = nn.Linear(c.ffn, c.hidden)
        self.ln2 = nn.LayerNorm(c.hidden, eps=c.ln_eps)
        self.heads = c.heads

    def forward_packed(self, x: torch.Tensor, cu: torch.Tensor, max_len: int) -> torch.Tensor:
        """x: [total_tokens, H] (sequences packed back to back), cu: int32 cumulative lengths [n+1]."""
        import os

        from torch.nn.attention.varlen import varlen_attn

        tot, h = x.shape
        if h != 384 or os.environ.get("LEANN_MI355X_GEMM") == "2" or (tot <= small_tokens_limit() and "LEANN_MI355X_GEMM" not in os.environ):
            # general widths (768: bge-base, contriever): five launches of the general MFMA GEMM + attention + two LayerNorms, no
            # library call -- QKV | attention | out-projection (+ residual) | LayerNorm | fc1 (+ GELU) | fc2 (+ residual) | LayerNorm.
            # Hidden 384 takes this form for SMALL forwards (<= LM_BERT_SMALL_TOKENS tokens: a one-query search round recomputes ~10
            # chunks): many small workgroups over the chip instead of the fused tail's one ~77 us workgroup chain (MI355X: B = 1
            # search p50 59.7 -> 47.2 ms at a limit of 6144 tokens, 44.9 -> 39.3 ms with the limit moved to 16384);
            # LEANN_MI355X_GEMM=2 forces it at every size (A/B), =1 / =0 keep the fused kernels.
            y = self._forward_packed_general(x, cu, max_len)
            if y is not None:
                return y
        a = None
        qkv_gemm = h == 384 and tot <= qkv_gemm_tokens_limit() and os.environ.get("LEANN_MI355X_FUSED_QKV_ATTN") != "1"  # (as csrc/lm_encoder_forward.cpp)
        if h == 384 and not qkv_gemm and os.environ.get("LEANN_MI355X_GEMM") != "1" and os.environ.get("LEANN_MI355X_LINEAR", "1") != "0" and os.environ.get("LEANN_MI355X_QKV", "1") == "1":
            a = fused_qkv_attention(x, self.qkv, cu, self.heads, max_len)  # projection fused into attention (forwards of long sequences)
        if a is None:
            qkv2 = (fused_gemm(x, self.qkv) if (qkv_gemm or os.environ.get("LEANN_MI355X_GEMM") == "1") else None) if h == 384 else None
            if qkv2 is None:
                qkv2 = fused_linear_h384(x, self.qkv)
            if qkv2 is None:
                qkv2 = self.qkv(x)
            a = fused_attention_hd32(qkv2, cu, self.heads, max_len)
            if a is None:
                qkv = qkv2.view(tot, 3, self.heads, h // self.heads)
                a = varlen_attn(qkv[:, 0], qkv[:, 1], qkv[:, 2], cu, cu, max_len, max_len).reshape(tot, h)
        y = fused_attn_out_mlp(a, x, self)  # output projection + LayerNorm + feed-forward block + LayerNorm in one kernel
        if y is not None:
            return y
        y = fused_linear_h384(a, self.out, residual=x, ln=self.ln1)
        x = y if y is not None else fused_add_layernorm(self.out(a), x, self.ln1)
        hmid = fused_gemm(x, self.fc1, GEMM_EPI_GELU)  # a feed-forward width outside the fused tail's envelope, or LEANN_MI355X_TAIL=0
        y = fused_gemm(hmid, self.fc2, GEMM_EPI_RESIDUAL, x) if hmid is not None else None
        if y is not None:
            return fused_add_layernorm(y, None, self.ln2)
        return fused_add_layernorm(self.fc2(F.gelu(self.fc1(x))), x, self.ln2)

    def _forward_packed_general(self, x: torch.Tensor, cu: torch.Tensor, max_len: int) -> Optional[torch.Tensor]:
        """The layer on the general kernels (lm_gemm_f16 + lm_attn_varlen_f16 + lm_add_layernorm_f16); None = a shape outside their
        envelope (the caller takes the library path)."""
        qkv = fused_gemm(x, self.qkv)
        if qkv is None:
            return None
        a = fused_attention_hd32(qkv, cu, self.heads, max_len)
        if a is None:
            return None
        y = fused_gemm(a, self.out, GEMM_EPI_RESIDUAL, x)
        if y is None:
            return None
        x1 = fused_add_layernorm(y, None, self.ln1)
        if x1 is None:  # LEANN_MI355X_LN=0 / a width outside the LayerNorm kernel's envelope: the torch LayerNorm
            x1 = self.ln1(y)
        hmid = fused_gemm(x1, self.fc1, GEMM_EPI_GELU)
        y2 = fused_gemm(hmid, self.fc2, GEMM_EPI_RESIDUAL, x1) if hmid is not None else None
        if y2 is None:
            return None
        out = fused_add_layernorm(y2, None, self.ln2)
        return out if out is not None else self.ln2(y2)

    def forward(self, x: torch.Tensor, mask: Optional[torch.Tensor]) -> torch.Tensor:
        n, t, h = x.shape
        qkv = self.qkv(x).view(n, t, 3, self.heads, h // self.heads).permute(2, 0, 3, 1, 4)
        a = F.scaled_dot_product_attention(qkv[0], qkv[1], qkv[2], attn_mask=mask)
        a = a.transpose(1, 2).reshape(n, t, h)
        x = fused_add_layernorm(self.out(a), x, self.ln1)
        x = fused_add_layernorm(self.fc2(F.gelu(self.fc1(x))), x, self.ln2)
        return x


class BertEncoder(nn.Module):
    """BERT encoder + sentence pooling.  ``forward(input_ids[n,T], lengths[n]) -> [n, hidden] fp32``."""

    weights_source = "unset"  # "checkpoint" | "random": which tokenizers are admissible (tokenizer.load_tokenizer)

    def __init__(self, cfg: EncoderConfig):
        super().__init__()
        self.cfg = cfg
        self.word = nn.Embedding(cfg.vocab_size, cfg.hidden)
        self.pos = nn.Embedding(cfg.max_pos, cfg.hidden)
        self.tok_type = nn.Embedding(cfg.type_vocab, cfg.hidden)
        self.ln = nn.LayerNorm(cfg.hidden, eps=cfg.ln_eps)
        self.layers = nn.ModuleList([_Layer(cfg) for _ in range(cfg.layers)])

    # ---- construction ----------------------------------------------------------------------
    @classmethod
    def random_init(cls, cfg: EncoderConfig, seed: int = 0) -> "BertEncoder":
        """Seeded Hugging Face-style init (normal(0, 0.02) weights, zero biases, unit LayerNorm),
        generated on the CPU so that every device gets identical bits."""
        g = torch.Generator(device="cpu").manual_seed(seed)
        m = cls(cfg)
        with torch.no_grad():
            for mod in m.modules():
                if isinstance(mod, (nn.Linear, nn.Embedding)):
                    mod.weight.copy_(torch.randn(mod.weight.shape, generator=g) * 0.02)
                    if isinstance(mod, nn.Linear):
                        mod.bias.zero_()
                elif isinstance(mod, nn.LayerNorm):
                    mod.weight.fill_(1.0)
                    mod.bias.zero_()
        m.weights_source = "random"
        return m.eval()

    @classmethod
    def from_hf_state_dict(cls, cfg: EncoderConfig, sd: dict) -> "BertEncoder":
        """Load a Hugging Face ``BertModel`` state dict (the module sentence-transformers wraps)."""
        sd = {k[len("bert."):] if k.startswith("bert.") else k: v for k, v in sd.items()}
        m = cls(cfg)
        with torch.no_grad():
            m.word.weight.copy_(sd["embeddings.word_embeddings.weight"])
            m.pos.weight.copy_(sd["embeddings.position_embeddings.weight"])
            m.tok_type.weight.copy_(sd["embeddings.token_type_embeddings.weight"])
            m.ln.weight.copy_(sd["embeddings.LayerNorm.weight"])
            m.ln.bias.copy_(sd["embeddings.LayerNorm.bias"])
            for i, L in enumerate(m.layers):
                p = f"encoder.layer.{i}."
                L.qkv.weight.copy_(torch.cat([sd[p + f"attention.self.{n}.weight"] for n in ("query", "key", "value")], 0))
                L.qkv.bias.copy_(torch.cat([sd[p + f"attention.self.{n}.bias"] for n in ("query", "key", "value")], 0))
                L.out.weight.copy_(sd[p + "attention.output.dense.weight"])
                L.out.bias.copy_(sd[p + "attention.output.dense.bias"])
                L.ln1.weight.copy_(sd[p + "attention.output.LayerNorm.weight"])
                L.ln1.bias.copy_(sd[p + "attention.output.LayerNorm.bias"])
                L.fc1.weight.copy_(sd[p + "intermediate.dense.weight"])
                L.fc1.bias.copy_(sd[p + "intermediate.dense.bias"])
                L.fc2.weight.copy_(sd[p + "output.dense.weight"])
                L.fc2.bias.copy_(sd[p + "output.dense.bias"])
                L.ln2.weight.copy_(sd[p + "output.LayerNorm.weight"])
                L.ln2.bias.copy_(sd[p + "output.LayerNorm.bias"])
        m.weights_source = "checkpoint"
        return m.eval()

    @classmethod
    def load(cls, model_name: str, seed: int = 0, allow_random: bool = False) -> "BertEncoder":
        """Weights of a local Hugging Face BERT checkpoint (``model_name`` = a directory, or a hub id present in the
        offline HF cache).  Pooling / normalisation / max_seq_length come from the checkpoint's own
        sentence-transformers files when it has them, else from the name preset (strict: unknown names raise).

        No silent fallback: a checkpoint that cannot be loaded, or one that is not a plain BERT (``model_type !=
        "bert"``: MPNet, XLM-R ... have different state dicts), raises.  ``allow_random=True`` -- tests, the synthetic
        benchmark, kernel autotuning: anything that measures throughput or compares the GPU path with itself --
        instead returns seeded random weights of the preset architecture when no checkpoint is available."""
        import logging

        log = logging.getLogger(__name__)
        try:
            from transformers import AutoConfig, AutoModel

            hc = AutoConfig.from_pretrained(model_name, local_files_only=True)
        except Exception as ex:  # noqa: BLE001 - not in the offline cache / not a checkpoint directory
            if allow_random:
                log.warning(f"embedding model {model_name!r}: no local checkpoint ({type(ex).__name__}); "
                            "using SEEDED RANDOM weights of the preset architecture (allow_random=True)")
                return cls.random_init(config_for(model_name), seed)
            raise RuntimeError(
                f"embedding model {model_name!r} is not available locally ({type(ex).__name__}: {ex}). Recompute search needs the "
                "weights the index was built with; pass a checkpoint directory, or allow_random=True for synthetic runs.") from ex
        if getattr(hc, "model_type", None) != "bert":
            raise RuntimeError(f"embedding model {model_name!r} has model_type={getattr(hc, 'model_type', None)!r}; only BERT-architecture "
                               "checkpoints (all-MiniLM, bge, contriever ...) are supported by the MI355X encoder")
        hf = AutoModel.from_pretrained(model_name, local_files_only=True)
        mdir = Path(model_name) if Path(model_name).is_dir() else Path(getattr(hf, "name_or_path", "") or "")
        st = sentence_transformers_settings(mdir) if mdir.is_dir() else {}
        if not {"pooling", "normalize"} <= set(st):  # hub-cache snapshot without the ST files: fall back to the name preset
            try:
                from huggingface_hub import snapshot_download

                st = {**sentence_transformers_settings(Path(snapshot_download(model_name, local_files_only=True))), **st}
            except Exception:  # noqa: BLE001
                pass
        base = config_for(model_name, strict=not {"pooling", "normalize"} <= set(st))
        cfg = replace(base, vocab_size=hc.vocab_size, hidden=hc.hidden_size, layers=hc.num_hidden_layers,
                      heads=hc.num_attention_heads, ffn=hc.intermediate_size, max_pos=hc.max_position_embeddings,
                      type_vocab=hc.type_vocab_size, ln_eps=hc.layer_norm_eps, **st)
        log.info(f"embedding model {model_name!r}: loaded checkpoint weights (pooling={cfg.pooling}, normalize={cfg.normalize}, "
                 f"max_seq_length={cfg.max_seq_length})")
        return cls.from_hf_state_dict(cfg, hf.state_dict())

    # ---- forward ---------------------------------------------------------------------------
    def forward(self, input_ids: torch.Tensor, lengths: torch.Tensor) -> torch.Tensor:
        cfg = self.cfg
        n, t = input_ids.shape
        pos = torch.arange(t, device=input_ids.device)
        x = self.word(input_ids) + self.pos(pos)[None] + self.tok_type.weight[0][None, None]
        x = self.ln(x)
        valid = pos[None, :] < lengths[:, None]  # [n, t]
        mask = None
        if not bool((lengths == t).all()):
            mask = valid[:, None, None, :]  # broadcast over heads and query positions
        for L in self.layers:
            x = L(x, mask)
        x = x.float()
        if cfg.pooling == "cls":
            e = x[:, 0]
        else:  # mean over valid tokens (sentence-transformers Pooling / embedding_compute.py:323-334)
            w = valid.unsqueeze(-1).to(x.dtype)
            e = (x * w).sum(1) / w.sum(1).clamp(min=1e-9)
        if cfg.normalize:
            e = F.normalize(e, p=2, dim=1)
        return e

    # ---- packed (padding-free) path: varlen flash attention, every other op on [total_tokens, H] ----
    _varlen_ok: Optional[bool] = None  # resolved on first use (per process)

    def onecall_model(self) -> Optional[dict]:
        """``{"model": lm_bert_h384 struct, ...}`` over this encoder's weights (packed copies cached, rebuilt when a weight changes: _packed)
        -- the argument of lm_bert_h384_forward_packed and of the built-in recompute provider (lm_recompute_create) -- or None when the
        model is outside that envelope: needs hidden 384 = heads x 32, fp16 weights ON THE GPU (checked: the weight images are written by device kernels), mean or CLS pooling, ffn a multiple of 192 in
        [192, 1728] (the fused layer tail's shapes; other widths: general_model)."""
        cfg = self.cfg
        w = self.word.weight
        if not (w.is_cuda and w.dtype == torch.float16 and cfg.hidden == 384 and cfg.heads * 32 == 384 and cfg.pooling in ("mean", "cls")
                and cfg.ffn % 192 == 0 and 192 <= cfg.ffn <= 1728):
            return None
        import os

        qkv_streaming = os.environ.get("LEANN_MI355X_QKV", "1") == "1"  # part of the pack's identity: read per call, one cached pack per form

        from . import _lib

        def make():
            keep, layers = [], (_lib.BertH384Layer * cfg.layers)()
            ptr = lambda t: (keep.append(t), t.data_ptr())[1]  # noqa: E731 - tensors stay referenced for the life of the pack
            for li, L in enumerate(self.layers):
                wo_i, w1_i, w2_i = pack_tail_images(L.out.weight, L.fc1.weight, L.fc2.weight)
                vals = (L.qkv.weight.detach().contiguous(), L.qkv.bias.detach().float().contiguous(), wo_i,
                        L.out.bias.detach().float().contiguous(), L.ln1.weight.detach().contiguous(), L.ln1.bias.detach().contiguous(),
                        w1_i, L.fc1.bias.detach().float().contiguous(), w2_i,
                        L.fc2.bias.detach().float().contiguous(), L.ln2.weight.detach().contiguous(), L.ln2.bias.detach().contiguous(),
                        L.out.weight.detach().contiguous(), L.fc1.weight.detach().contiguous(), L.fc2.weight.detach().contiguous(),
                        pack_qkv_image(L.qkv.weight) if qkv_streaming else None)
                for (name, _), v in zip(_lib.BertH384Layer._fields_, vals):
                    setattr(layers[li], name, ptr(v) if v is not None else None)
            m = _lib.BertH384(cfg.layers, cfg.heads, cfg.ffn, 1 if cfg.normalize else 0, 1 if cfg.pooling == "cls" else 0, float(self.ln.eps), ptr(w.detach()),
                              ptr(self.pos.weight.detach()), ptr(self.tok_type.weight[0].detach().contiguous()), ptr(self.ln.weight.detach()),
                              ptr(self.ln.bias.detach()), layers)
            return {"model": m, "layers": layers, "keep": keep}

        return _packed(self, "_onecall_pack" if qkv_streaming else "_onecall_pack_ws_qkv", tuple(self.parameters()), make)

    def general_model(self) -> Optional[dict]:
        """``{"model": lm_bert struct, ...}`` over this encoder's own (unpacked) weights: the argument of lm_bert_forward_packed and
        lm_recompute_create_general -- every width the general kernels take (hidden % 128 == 0 and <= 768, ffn % 128 == 0, head_dim 32
        or 64, mean or CLS pooling, fp16): bge-base, contriever.  None outside that envelope."""
        cfg = self.cfg
        w = self.word.weight
        hd = cfg.hidden // cfg.heads if cfg.heads else 0
        if not (w.dtype == torch.float16 and cfg.hidden % 128 == 0 and cfg.hidden <= 768 and cfg.ffn % 128 == 0 and hd * cfg.heads == cfg.hidden
                and hd in (32, 64) and cfg.pooling in ("mean", "cls")):
            return None
        from . import _lib

        def make():
            keep, layers = [], (_lib.BertLayer * cfg.layers)()
            ptr = lambda t: (keep.append(t), t.data_ptr())[1]  # noqa: E731 - tensors stay referenced for the life of the pack
            for li, L in enumerate(self.layers):
                vals = (L.qkv.weight.detach().contiguous(), L.qkv.bias.detach().float().contiguous(), L.out.weight.detach().contiguous(),
                        L.out.bias.detach().float().contiguous(), L.ln1.weight.detach().contiguous(), L.ln1.bias.detach().contiguous(),
                        L.fc1.weight.detach().contiguous(), L.fc1.bias.detach().float().contiguous(), L.fc2.weight.detach().contiguous(),
                        L.fc2.bias.detach().float().contiguous(), L.ln2.weight.detach().contiguous(), L.ln2.bias.detach().contiguous())
                for (name, _), v in zip(_lib.BertLayer._fields_, vals):
                    setattr(layers[li], name, ptr(v))
            m = _lib.Bert(cfg.hidden, cfg.layers, cfg.heads, cfg.ffn, 1 if cfg.pooling == "cls" else 0, 1 if cfg.normalize else 0, float(self.ln.eps),
                          ptr(w.detach()), ptr(self.pos.weight.detach()), ptr(self.tok_type.weight[0].detach().contiguous()),
                          ptr(self.ln.weight.detach()), ptr(self.ln.bias.detach()), layers)
            return {"model": m, "layers": layers, "keep": keep}

        return _packed(self, "_general_pack", tuple(self.parameters()), make)

    def _forward_one_call(self, tok: torch.Tensor, pos: torch.Tensor, cu: torch.Tensor, max_len: int) -> Optional[torch.Tensor]:
        """The whole packed forward as ONE call into the library (csrc/lm_encoder_forward.cpp: lm_bert_h384_forward_packed) -- the same
        kernels as the per-kernel path below, strung together on the C++ side, so a recompute round costs one ctypes call instead of
        ~3 L + 2.  Default since round 3 (measured on an MI355X, 200k-chunk index: B = 1 p50 57.7 -> 56.3 ms, B = 4 68.2 -> 66.8 ms;
        bit-identical results); LEANN_MI355X_ONECALL=0 = the per-kernel path (A/B).  Applies to hidden 384 = heads x 32, fp16, mean
        pooling, lengths <= 512, no kernel-selection switch set (KERNEL_SELECTION_KEYS), no per-kernel timers running.  None = not
        applicable: the caller takes the per-kernel path (logged once per reason)."""
        import os

        if os.environ.get("LEANN_MI355X_ONECALL", "1") != "1" or KernelTimers.active is not None:
            return None
        ab = [k for k in KERNEL_SELECTION_KEYS if k in os.environ]
        if ab:  # an A/B run of a particular kernel generation goes through the per-kernel path
            self._log_declined(f"kernel-selection switches set ({', '.join(ab)})")
            return None
        if not (tok.is_cuda and 0 < max_len <= 512 and tok.dtype == torch.int32 and pos.dtype == torch.int32 and cu.dtype == torch.int32):
            return None
        import ctypes as C

        from . import _lib

        lib = _lib.load()
        tot, n = tok.shape[0], cu.shape[0] - 1
        pk = self.onecall_model()
        if pk is None:  # other widths (768: bge-base, contriever): the general kernels, also strung together on the C++ side
            gk = self.general_model()
            if gk is None:
                return None
            need = int(lib.lm_bert_workspace_bytes(C.byref(gk["model"]), tot))
            ws = getattr(self, "_onecall_ws", None)
            if ws is None or ws.device != tok.device or ws.numel() < need:
                ws = torch.empty((max(need, 1 << 20),), dtype=torch.uint8, device=tok.device)
                self._onecall_ws = ws
            out = torch.empty((n, self.cfg.hidden), dtype=torch.float32, device=tok.device)
            _lib.check(lib.lm_bert_forward_packed(C.byref(gk["model"]), C.c_void_p(tok.data_ptr()), C.c_void_p(pos.data_ptr()), C.c_void_p(cu.data_ptr()),
                                                  n, tot, int(max_len), C.c_void_p(ws.data_ptr()), ws.numel(), C.c_void_p(out.data_ptr()),
                                                  C.c_void_p(torch.cuda.current_stream(tok.device).cuda_stream)), "lm_bert_forward_packed")
            return out
        need = int(lib.lm_bert_h384_workspace_bytes(tot))
        ws = getattr(self, "_onecall_ws", None)
        if ws is None or ws.device != tok.device or ws.numel() < need:
            ws = torch.empty((max(need, 1 << 20),), dtype=torch.uint8, device=tok.device)
            self._onecall_ws = ws
        out = torch.empty((n, 384), dtype=torch.float32, device=tok.device)
        _lib.check(lib.lm_bert_h384_forward_packed(C.byref(pk["model"]), C.c_void_p(tok.data_ptr()), C.c_void_p(pos.data_ptr()), C.c_void_p(cu.data_ptr()),
                                                   n, tot, int(max_len), C.c_void_p(ws.data_ptr()), ws.numel(), C.c_void_p(out.data_ptr()),
                                                   C.c_void_p(torch.cuda.current_stream(tok.device).cuda_stream)), "lm_bert_h384_forward_packed")
        return out

    def _log_declined(self, why: str) -> None:
        seen = self.__dict__.setdefault("_declined_logged", set())
        if why not in seen:
            seen.add(why)
            import logging

            logging.getLogger(__name__).info(f"one-call forward not used: {why}; taking the per-kernel path")

    def forward_packed(self, tok: torch.Tensor, pos: torch.Tensor, cu: torch.Tensor, seq_of: torch.Tensor,
                       lengths: torch.Tensor, max_len: int) -> torch.Tensor:
        cfg = self.cfg
        one = self._forward_one_call(tok, pos, cu, max_len)
        if one is not None:
            return one
        x = fused_embed_layernorm(tok, pos, self.word, self.pos, self.tok_type.weight[0], self.ln)
        if x is None:
            x = fused_add_layernorm(self.word(tok) + self.tok_type.weight[0][None], self.pos(pos), self.ln)
        for L in self.layers:
            x = L.forward_packed(x, cu, max_len)
        n = lengths.shape[0]
        e = fused_meanpool(x, cu, cfg.normalize, cls=cfg.pooling == "cls")  # mean or CLS (+ normalisation) in one kernel
        if e is not None:
            return e
        if cfg.pooling == "cls":
            e = x[cu[:-1].long()].float()
        else:
            if seq_of is None:  # packed front end: only this path needs the token -> sequence map
                seq_of = torch.repeat_interleave(torch.arange(n, device=x.device), lengths.long(), output_size=x.shape[0])
            e = torch.zeros((n, cfg.hidden), dtype=torch.float32, device=x.device).index_add_(0, seq_of, x.float())
            e = e / lengths.clamp(min=1).unsqueeze(1).float()
        if cfg.normalize:
            e = F.normalize(e, p=2, dim=1)
        return e

    @torch.no_grad()
    def encode_tokens_packed(self, input_ids: torch.Tensor, lengths: torch.Tensor, max_tokens: int = 262144) -> torch.Tensor:
        """No padding anywhere: sequences are concatenated; sub-batches are cut by token budget.  Host-side cost matters here: a
        one-query search calls this ~100 times with a handful of chunks, so the preamble is three small device ops (zeros, cumsum,
        copy) and ONE device-to-host copy (the cumulative lengths: sub-batch bounds and allocation sizes come from that array)."""
        n, t = input_ids.shape
        out = torch.empty((n, self.cfg.hidden), dtype=torch.float32, device=input_ids.device)
        if n == 0:
            return out
        cu_all = torch.zeros(n + 1, dtype=torch.int32, device=input_ids.device)
        cu_all[1:] = torch.cumsum(lengths, 0)
        cs_np = cu_all.cpu().numpy().astype(np.int64)  # the one host sync of the forward
        lens_np = np.diff(cs_np)
        # sub-batch boundaries by cumulative token count
        bounds = [0]
        while bounds[-1] < n:
            j = int(np.searchsorted(cs_np[1:], cs_np[bounds[-1]] + max_tokens, side="right"))
            j = min(max(j, bounds[-1] + 1), n)
            bounds.append(j)
        import os

        pack_on = os.environ.get("LEANN_MI355X_PACK", "1") == "1"  # packed front end in one kernel (fused_pack_tokens)
        ar = None
        for b0, b1 in zip(bounds[:-1], bounds[1:]):
            ids = input_ids[b0:b1]
            ln = lengths[b0:b1]
            cu = cu_all if (b0 == 0 and b1 == n) else (cu_all[b0 : b1 + 1] - cu_all[b0]).contiguous()
            total = int(cs_np[b1] - cs_np[b0])
            max_len = int(lens_np[b0:b1].max())
            if pack_on and ln.dtype == torch.int32:
                packed = fused_pack_tokens(ids, ln, cu, total)
                if packed is not None:
                    e = self.forward_packed(packed[0], packed[1], cu, None, ln, max_len)
                    if b0 == 0 and b1 == n:
                        return e
                    out[b0:b1] = e
                    continue
            if ar is None:
                ar = torch.arange(t, device=input_ids.device)
            valid = ar[None, :] < ln[:, None]
            tok = ids[valid]
            pos = ar[None, :].expand(b1 - b0, t)[valid]
            seq_of = torch.arange(b1 - b0, device=ids.device)[:, None].expand(b1 - b0, t)[valid]
            out[b0:b1] = self.forward_packed(tok, pos, cu, seq_of, ln, max_len)
        return out

    @torch.no_grad()
    def encode_tokens(self, input_ids: torch.Tensor, lengths: torch.Tensor, batch_size: int = 1024,
                      bucket: int = 32) -> torch.Tensor:
        """Packed varlen path when the build supports it on this device (GPU, fp16/bf16), else the
        length-bucketed padded path below."""
        if input_ids.is_cuda and self.word.weight.dtype in (torch.float16, torch.bfloat16):
            if BertEncoder._varlen_ok is None:
                try:
                    self.encode_tokens_packed(input_ids[:2], lengths[:2])
                    BertEncoder._varlen_ok = True
                except Exception:  # noqa: BLE001 - varlen flash attention unavailable in this build
                    BertEncoder._varlen_ok = False
            if BertEncoder._varlen_ok:
                return self.encode_tokens_packed(input_ids, lengths, max_tokens=batch_size * 192)
        return self.encode_tokens_padded(input_ids, lengths, batch_size, bucket)

    @torch.no_grad()
    def encode_tokens_padded(self, input_ids: torch.Tensor, lengths: torch.Tensor, batch_size: int = 1024,
                             bucket: int = 32) -> torch.Tensor:
        """Length-bucketed batched forward: rows are grouped by ceil(len/bucket) and every group
        is truncated to its own max length, so padding waste is < bucket tokens per chunk."""
        n = input_ids.shape[0]
        out = torch.empty((n, self.cfg.hidden), dtype=torch.float32, device=input_ids.device)
        if n == 0:
            return out
        order = torch.argsort(lengths, stable=True)
        sl = lengths[order]
        # group boundaries where the bucketed length changes or the batch is full
        bl = ((sl + bucket - 1) // bucket).tolist()
        start = 0
        while start < n:
            end = start + 1
            while end < n and end - start < batch_size and bl[end] == bl[start]:
                end += 1
            idx = order[start:end]
            tmax = int(sl[end - 1])
            out[idx] = self.forward(input_ids[idx, :tmax], lengths[idx])
            start = end
        return out


def hf_reference_embed(hf_model, input_ids: torch.Tensor, lengths: torch.Tensor, pooling: str, normalize: bool):
    """sentence-transformers semantics on top of a Hugging Face BertModel (used by the parity tests
    and the golden-vector generator)."""
    t = input_ids.shape[1]
    mask = (torch.arange(t)[None, :] < lengths[:, None]).long()
    with torch.no_grad():
        h = hf_model(input_ids=input_ids.long(), attention_mask=mask).last_hidden_state.float()
    if pooling == "cls":
        e = h[:, 0]
    else:
        w = mask.unsqueeze(-1).float()
        e = (h * w).sum(1) / w.sum(1).clamp(min=1e-9)
    return F.normalize(e, p=2, dim=1) if normalize else e
