"""lm_pq_encode / lm_pq_train -- the product quantiser's assignment and Lloyd iterations as HIP kernels -- on the CPU: the product library
built for the host (tests/hip_emul/build_emul_lib.py, a thread per lane) against tests/pq_ref/lm_pq_ref.c, an independent C restatement
of the header's contract, and against argmin over the oracle's orc_pq_lut (the table the search reads).  The scenarios live in
tests/emulated_pq_build_cases.py and run in a child process that loads the emulated library."""
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CLANG = Path("/opt/rocm/lib/llvm/bin/clang++")
sys.path.insert(0, str(ROOT / "tests" / "hip_emul"))


@pytest.fixture(scope="module")
def libs(tmp_path_factory, built_libs):
    if not CLANG.exists():
        pytest.skip("needs ROCm's clang++ as a host compiler")
    import build_emul_lib

    from oracle import oracle as orc
    from tests.pq_ref_util import compile_ref

    orc.lib()  # the second pin reads orc_pq_lut from the oracle library (built on first use)
    d = tmp_path_factory.mktemp("emul_pq_build")
    return build_emul_lib.build(d), compile_ref(d)


def _run(libs, *cases, timeout=1800):
    r = subprocess.run([sys.executable, "-m", "tests.emulated_pq_build_cases", str(libs[0]), str(libs[1]), *cases], cwd=str(ROOT), capture_output=True,
                       text=True, timeout=timeout)
    assert r.returncode == 0 and "ALL CASES OK" in r.stdout, r.stdout[-3000:] + r.stderr[-5000:]
    assert "MISMATCH" not in r.stdout
    return r.stdout


def test_encode_matches_the_c_restatement_and_the_oracle_lut(libs):
    out = _run(libs, "encode_vs_restatement", "encode_ties_and_nan")
    assert out.count(": ok") >= 19


def test_train_matches_the_c_restatement_bit_for_bit(libs):
    out = _run(libs, "train_vs_restatement")
    assert out.count(": ok") >= 21


def test_kernel_and_torch_forms_agree_on_exact_arithmetic(libs):
    _run(libs, "agreement_with_the_torch_form")


def test_kernel_trained_quantiser_is_as_good_as_the_torch_form(libs):
    """Observed on the host build of the library: torch MSE by seed 0..4 35.7897 / 35.7762 / 35.6724 / 35.4508 / 35.5127 (spread 0.96 %);
    kernel form at seed 0 35.7900 = 1.000007 x the torch form's.  The case prints the figures before it asserts."""
    print(_run(libs, "quality_against_the_torch_form"))


def test_builders_take_gpu_pq_kernel(libs):
    _run(libs, "builder_wiring")


def test_rejected_arguments(libs):
    _run(libs, "argument_checking")


def test_default_quantiser_is_the_torch_pair():
    """The default does not change: gpu_pq_kernel defaults to False and the torch pair keeps its signature."""
    import inspect

    from leann_amd import backend, pq

    assert inspect.signature(backend._make_pq).parameters["gpu_pq_kernel"].default is False
    assert list(inspect.signature(pq.train_pq).parameters) == ["x", "m", "iters", "sample", "seed"]
    assert list(inspect.signature(pq.encode_pq).parameters) == ["x", "codebooks", "block"]
    assert [p.default for p in inspect.signature(pq.train_pq_kernel).parameters.values()][2:] == [12, 131072, 0]
