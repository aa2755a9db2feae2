"""lm_graph_levels_to_csr_count / _fill and lm_graph_csr_to_level on the CPU: the product library built for the host
(tests/hip_emul/build_emul_lib.py, a thread per lane) against the project's numpy assembly (tests/csr_ref_util.py).  The scenarios live
in tests/emulated_csr_cases.py and run in a child process that loads the emulated library."""
import inspect
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "hip_emul"))


@pytest.fixture(scope="module")
def lib(tmp_path_factory, built_libs):
    if not Path("/opt/rocm/lib/llvm/bin/clang++").exists():
        pytest.skip("needs ROCm's clang++ as a host compiler")
    import build_emul_lib

    return build_emul_lib.build(tmp_path_factory.mktemp("emul_csr"))


@pytest.mark.parametrize("case", ["kernel_vs_reference", "rejections", "builder_wiring"])
def test_emulated_case(lib, case):
    r = subprocess.run([sys.executable, "-m", "tests.emulated_csr_cases", str(lib), case], cwd=str(ROOT), capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0 and "ALL CASES OK" in r.stdout, r.stdout[-3000:] + r.stderr[-5000:]


def test_defaults_are_the_numpy_assembly():
    from leann_amd import gpu_graph_build as gb

    assert all(inspect.signature(f).parameters["assembler"].default == "numpy" for f in (gb.build_graph_gpu, gb.prune_preserving_hubs))
