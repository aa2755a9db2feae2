"""The composed encoder forward on a trained-shaped model (tests/encoder_ref_util.py) against fp64, run against libleann_mi355x_emul.so
(tests/hip_emul/build_emul_lib.py: the product's kernels on the CPU, a thread per lane).  Imported by tests/test_encoder_trained_like.py and runnable:
    python -m tests.emulated_encoder_cases <path/to/libleann_mi355x_emul.so> [case ...]
What this checks without a GPU is the marshalling: BertEncoder.onecall_model's positional fill of the per-layer struct, the launch sequences of
csrc/lm_encoder_forward.cpp and the per-kernel path of leann_amd/encoder.py, on weights where no two fields are interchangeable.  The bound is
2 x E0, E0 = max |plain torch fp16 forward - fp64| on the same weights.  Only test code pretends the tensors are device tensors."""
import os
import sys
from contextlib import contextmanager
from pathlib import Path
from unittest import mock

import numpy as np

CASES = {}
LENGTHS = [48, 47, 33, 32, 31, 17, 8, 2, 1]
FORMS = {  # name -> (environment, _lib.check names of the per-kernel launch path; 2 layers)
    "small": ({}, {"lm_gemm_f16": 8, "lm_attn_varlen_hd32_f16": 2, "lm_add_layernorm_f16": 4}),
    "pair": ({"LEANN_MI355X_SMALL_TOKENS": "0"}, {"lm_qkv_h384_f16": 2, "lm_attn_varlen_hd32_f16": 2, "lm_layer_tail_h384_f16": 2}),
    "fused": ({"LEANN_MI355X_SMALL_TOKENS": "0", "LEANN_MI355X_FUSED_QKV_ATTN": "1"}, {"lm_qkv_attn_h384_f16": 2, "lm_layer_tail_h384_f16": 2}),
}


def _load(lib_path: str):
    from leann_amd import _lib

    _lib.LIB_PATH = Path(lib_path)
    _lib._lib = None
    return _lib.load()


class _Stream:
    cuda_stream = 0


@contextmanager
def _device_world(env, used):
    import torch

    from leann_amd import _lib

    e = {k: v for k, v in os.environ.items() if not k.startswith("LEANN_MI355X_")}
    e.update(env)
    real = _lib.check

    def recording(rc, what=""):
        used.append(what)
        return real(rc, what)

    with mock.patch.object(torch.Tensor, "is_cuda", new=property(lambda self: True)), mock.patch("torch.cuda.current_stream", new=lambda *a, **k: _Stream()), \
            mock.patch.dict(os.environ, e, clear=True), mock.patch.object(_lib, "check", new=recording), torch.no_grad():
        yield


def _world():
    from tests import encoder_ref_util as U

    cfg = U.minilm_cfg(vocab=500, layers=2, ffn=384, max_pos=64)
    enc = U.trained_like_init(cfg, 4).half()
    ids, lens = U.make_batch(cfg, LENGTHS, 6)
    return U, cfg, enc, ids, lens


def _forward(enc, ids, lens, env, used):
    used.clear()
    with _device_world(env, used):
        return enc.encode_tokens_packed(ids, lens, 4096).clone()


def _bound(U, tag, got, ref, e0):
    err, cos = U.errors(got, ref)
    ok = np.isfinite(err) and err <= 2.0 * e0 and cos >= 0.9999
    print(f"{tag}: max|diff| vs fp64 {err:.3e} = {err / e0:.2f} x E0 ({e0:.3e}), min cosine {cos:.7f}: {'within 2 x E0' if ok else 'OUTSIDE'}", flush=True)
    assert ok, (tag, err, e0, cos)


def case_forms():
    """The one-call forward in its small form, as the head-major pair + layer tail and with the fused first half, and the per-kernel path of each
    (same bits), against fp64."""
    import torch

    U, cfg, enc, ids, lens = _world()
    ref = U.reference_fp64(enc, ids, lens)
    e0, cos0 = U.errors(U.plain_fp16(enc, ids, lens), ref)
    print(f"E0 (plain torch fp16 vs fp64): {e0:.3e}, min cosine {cos0:.7f}", flush=True)
    assert cos0 >= 0.9999
    used = []
    for form, (env, names) in FORMS.items():
        one = _forward(enc, ids, lens, env, used)
        assert used.count("lm_bert_h384_forward_packed") == 1 and not any(n in used for n in names), (form, sorted(set(used)))
        _bound(U, f"one call, form {form}", one, ref, e0)
        per = _forward(enc, ids, lens, {**env, "LEANN_MI355X_ONECALL": "0"}, used)
        assert "lm_bert_h384_forward_packed" not in used and {k: used.count(k) for k in names} == names, (form, sorted(set(used)))
        assert torch.equal(one, per), (form, float((one - per).abs().max()))
        _bound(U, f"per kernel, form {form}", per, ref, e0)


CASES["forms"] = case_forms


def case_sensitivity():
    """Two parameter tensors changed in place, one at a time (layer 1's out.bias, layer 0's ln2.bias: the fields the wiring mutants of
    tests/encoder_ref_util.py exchange): the small and the large one-call forward follow the fp64 reference of the changed weights -- a stale packed
    copy or a field read from the wrong slot does not."""
    import torch

    U, cfg, enc, ids, lens = _world()
    used = []
    base = {f: _forward(enc, ids, lens, FORMS[f][0], used) for f in ("small", "pair")}
    for step, (name, li) in enumerate((("out.bias", 1), ("ln2.bias", 0))):
        p = dict(enc.named_parameters())[f"layers.{li}.{name}"]
        delta = 0.3 * torch.randn(p.shape, generator=torch.Generator().manual_seed(70 + step))
        with torch.no_grad():
            p.add_(delta.to(p.dtype))
        ref = U.reference_fp64(enc, ids, lens)
        e0, _ = U.errors(U.plain_fp16(enc, ids, lens), ref)
        for f in ("small", "pair"):
            got = _forward(enc, ids, lens, FORMS[f][0], used)
            _bound(U, f"layer {li} {name} changed, form {f}", got, ref, e0)
            moved = float((got - base[f]).abs().max())
            print(f"    moved by {moved:.3e}", flush=True)
            assert moved > 2.0 * e0, (name, f, moved, e0)
            base[f] = got


CASES["sensitivity"] = case_sensitivity


if __name__ == "__main__":
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    _load(sys.argv[1])
    import time

    import torch

    torch.set_num_threads(1)
    for name in (sys.argv[2:] or list(CASES)):
        t0 = time.time()
        CASES[name]()
        print(f"[case {name}: {time.time() - t0:.1f} s]", flush=True)
    print("ALL CASES OK")
