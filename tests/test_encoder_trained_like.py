"""The trained-shaped encoder of tests/encoder_ref_util.py on the CPU: (1) the model and the batch the GPU tests use really hold the features they are
for -- sharp attention, the deferred-rescale condition, GELU inputs beyond +-3, no interchangeable parameter -- and the three wiring mutants move the
fp64 reference by far more than fp16 rounding does; (2) the kernels' GELU polynomial, restated in numpy, meets over every finite fp16 input the
bound the GPU tests assert; (3) the composed forward in every launch form over the host build of the library (tests/hip_emul/build_emul_lib.py,
a thread per lane; scenarios in tests/emulated_encoder_cases.py, run in a child process) against fp64."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests import encoder_ref_util as U

ROOT = Path(__file__).resolve().parent.parent
CLANG = Path("/opt/rocm/lib/llvm/bin/clang++")
sys.path.insert(0, str(ROOT / "tests" / "hip_emul"))

LENGTHS = [256, 255, 224, 129, 33, 32, 2, 1, 180, 97, 64, 200]  # tests/test_gpu_encoder_trained_like.py: the same model, the same batch


@pytest.fixture(scope="module")
def model():
    import torch

    cfg = U.minilm_cfg()
    enc = U.trained_like_init(cfg, 0).half()  # the values the GPU model holds
    ids, lens = U.make_batch(cfg, LENGTHS, 1)
    ref = U.reference_fp64(enc, ids, lens)
    e0, cos0 = U.errors(U.plain_fp16(enc, ids, lens), ref)
    return {"cfg": cfg, "enc": enc, "ids": ids, "lens": lens, "ref": ref, "e0": e0, "cos0": cos0}


def test_no_two_parameter_tensors_alike_no_zero_bias_no_unit_gamma(model):
    import torch

    enc, cfg = model["enc"], model["cfg"]
    again = U.trained_like_init(cfg, 0).half()
    assert all(torch.equal(a, b) for a, b in zip(enc.state_dict().values(), again.state_dict().values()))  # seeded
    other = U.trained_like_init(cfg, 1).half()
    assert not torch.equal(enc.layers[0].qkv.weight, other.layers[0].qkv.weight)
    for name in U.LAYER_TENSORS:
        ts = [dict(L.named_parameters())[name] for L in enc.layers]
        for i in range(cfg.layers):
            for j in range(i + 1, cfg.layers):
                assert float((ts[i].detach().float() - ts[j].detach().float()).abs().max()) > 0.05, (name, i, j)
    # tensors of one shape inside a layer (what a positional fill can swap) differ as well
    for L in enc.layers:
        same_shape = [L.out.bias, L.fc2.bias, L.ln1.weight, L.ln1.bias, L.ln2.weight, L.ln2.bias]
        for i in range(len(same_shape)):
            for j in range(i + 1, len(same_shape)):
                assert float((same_shape[i].detach().float() - same_shape[j].detach().float()).abs().max()) > 0.05
    for n, p in enc.named_parameters():
        if n.endswith(".bias"):
            assert bool((p != 0).all()), n
        if n.startswith("ln") or ".ln" in n:
            if n.endswith(".weight"):
                assert bool((p != 1).all()), n


def test_the_reference_forward_is_the_encoders_own_fp64_forward(model):
    """tests/encoder_ref_util.py writes the forward out op by op; the encoder's padded torch path on fp64 weights agrees with it up to
    that path's fp32 pooling."""
    import copy

    import torch

    with torch.no_grad():
        own = copy.deepcopy(model["enc"]).double()(model["ids"][:6], model["lens"][:6])
    assert float((own - model["ref"][:6]).abs().max()) < 2e-7


def test_the_batch_holds_the_features_the_gpu_tests_are_for(model):
    rows = U.describe(model["enc"], model["ids"], model["lens"])
    for li, r in enumerate(rows):
        print(f"layer {li}: " + ", ".join(f"{k} {v:.4g}" for k, v in r.items()))
    print(f"plain fp16 vs fp64: max|diff| {model['e0']:.3e}, min cosine {model['cos0']:.7f}")
    assert max(r["sharp"] for r in rows) >= 0.4 and min(r["sharp"] for r in rows) >= 0.01
    assert sum(r["grew"] for r in rows) >= 5
    assert all(r["fc1_below"] >= 0.01 and r["fc1_above"] >= 0.005 for r in rows)
    assert model["cos0"] >= 0.9999 and model["e0"] < 2e-3  # well conditioned for an fp16 pipeline: the 2 x E0 bound of the GPU tests means fp16 level


@pytest.mark.parametrize("mutant", list(U.MUTANTS))
def test_wiring_mutants_move_the_reference_far_beyond_fp16_level(model, mutant):
    moved = float((U.mutant_fp64(model["enc"], model["ids"], model["lens"], mutant) - model["ref"]).abs().max())
    print(f"{mutant}: embeddings move by {moved:.3e} = {moved / model['e0']:.1f} x the fp16-vs-fp64 distance {model['e0']:.3e}")
    assert moved > 4.0 * model["e0"]


def test_gelu_polynomial_meets_the_bound_over_every_finite_fp16_input():
    """The numpy restatement of gm_gelu / t4_gelu_uop: fp32 result within the kernels' stated 1e-6 of x Phi(x), fp16 result inside the bound the GPU
    sweep asserts (so that bound is attainable by the arithmetic the kernels document)."""
    x = U.all_finite_fp16()
    assert x.shape[0] == 63488
    p = U.gelu_poly_fp32(x.astype(np.float32))
    rep32 = U.gelu_sweep_report(x, p)
    rep16 = U.gelu_sweep_report(x, p.astype(np.float16))
    print("fp32:", rep32)
    print("fp16:", rep16)
    assert rep32["finite"] and rep32["abs"] <= 1e-6 and rep32["identity"]
    U.assert_gelu_sweep(rep16)
    # the checker is not vacuous: the tanh approximation of GELU, or one polynomial coefficient off in its 4th digit, is outside the bound
    xf = x.astype(np.float64)
    tanh = 0.5 * xf * (1.0 + np.tanh(0.7978845608028654 * (xf + 0.044715 * xf ** 3)))
    assert U.gelu_sweep_report(x, tanh.astype(np.float16))["excess"] > 0
    keep = U.GELU_COEFFS
    try:
        U.GELU_COEFFS = keep[:3] + (keep[3] * 1.0005,) + keep[4:]
        assert U.gelu_sweep_report(x, U.gelu_poly_fp32(x.astype(np.float32)).astype(np.float16))["excess"] > 0
    finally:
        U.GELU_COEFFS = keep


def test_layer_tail_gelu_sweep_bound_admits_the_documented_arithmetic():
    """tail_gelu_reference's bound against an fp32 emulation of what the layer tail computes for the sweep (polynomial GELU -> fp16, one-pass moments in
    fp32, fp16 output): inside; with a GELU that is 2 fp16 ulps off at one input: outside."""
    sweep = U.tail_gelu_sweep()
    assert sweep.shape == (1536,) and np.isfinite(sweep).all()
    for s in range(4):
        b1 = sweep[384 * s: 384 * (s + 1)]
        ref, bound = U.tail_gelu_reference(b1)
        v = U.gelu_poly_fp32(b1.astype(np.float32)).astype(np.float16).astype(np.float32)

        def kernel_ln(v):
            mean = np.float32(v.sum(dtype=np.float32) / np.float32(384))
            var = np.float32((v * v).sum(dtype=np.float32) / np.float32(384)) - mean * mean
            rstd = np.float32(1.0) / np.sqrt(var + np.float32(1e-12), dtype=np.float32)
            return (v * rstd - mean * rstd).astype(np.float16).astype(np.float64)

        assert (np.abs(kernel_ln(v) - ref) <= bound).all(), s
        if s < 3:
            j = int(np.argmin(np.abs(b1.astype(np.float64) - 1.0)))
            off = v.copy()
            off[j] += np.float32(2.0 * U.ulp16(float(v[j])))
            assert not (np.abs(kernel_ln(off) - ref) <= bound).all(), s


# ---- the composed forward over the host build of the library ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emul_lib(tmp_path_factory, built_libs):
    if not CLANG.exists():
        pytest.skip("needs ROCm's clang++ as a host compiler")
    import build_emul_lib

    return build_emul_lib.build(tmp_path_factory.mktemp("emul_encoder"))


def _run(lib, *cases, timeout=1800):
    r = subprocess.run([sys.executable, "-m", "tests.emulated_encoder_cases", str(lib), *cases], cwd=str(ROOT), capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and "ALL CASES OK" in r.stdout, r.stdout[-3000:] + r.stderr[-5000:]
    return r.stdout


def test_every_form_of_the_forward_against_fp64_on_the_host_build(emul_lib):
    out = _run(emul_lib, "forms")
    assert out.count("within 2 x E0") == 6  # one call and per kernel, three forms


def test_changed_parameter_tensors_on_the_host_build(emul_lib):
    _run(emul_lib, "sensitivity")
