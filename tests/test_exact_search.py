"""lm_exact_search -- exact top-k over a stored-embedding table with an allow-list, as HIP kernels -- on the CPU: the product library built for
the host (tests/hip_emul/build_emul_lib.py, a thread per lane) against the oracle's bruteforce_topk; labels equal, distance bits equal.  The
scenarios live in tests/emulated_exact_cases.py and run in a child process that loads the emulated library."""
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CLANG = Path("/opt/rocm/lib/llvm/bin/clang++")
sys.path.insert(0, str(ROOT / "tests" / "hip_emul"))


@pytest.fixture(scope="module")
def emul_lib(tmp_path_factory, built_libs):
    if not CLANG.exists():
        pytest.skip("needs ROCm's clang++ as a host compiler")
    import build_emul_lib

    return build_emul_lib.build(tmp_path_factory.mktemp("emul_exact"))


def _run(lib, *cases, timeout=1800):
    r = subprocess.run([sys.executable, "-m", "tests.emulated_exact_cases", str(lib), *cases], cwd=str(ROOT), capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and "ALL CASES OK" in r.stdout, r.stdout[-3000:] + r.stderr[-5000:]
    assert "MISMATCH" not in r.stdout
    return r.stdout


def test_kernel_matches_the_oracle_in_every_slicing_regime(emul_lib):
    out = _run(emul_lib, "kernel_vs_oracle")
    assert out.count(": ok") >= 80


def test_small_tables_nan_zero_and_ties_across_slices(emul_lib):
    _run(emul_lib, "small_tables_and_ties")


def test_allow_list_matches_the_oracle_on_the_compacted_table(emul_lib):
    _run(emul_lib, "allow_list")


def test_rejected_arguments_touch_nothing(emul_lib):
    _run(emul_lib, "argument_checking")


def test_index_exact_topk_kernel_and_backend_wiring(emul_lib):
    _run(emul_lib, "wiring")


def test_exact_is_off_by_default():
    """The default path does not change: Mi355xSearcher.search takes `exact` / `allowed_ids` through **kwargs only (absent = off), search_exact's
    allow-list defaults to None, exact_topk_ip keeps its signature."""
    import inspect

    from leann_amd import backend, exact
    from leann_amd.index import Mi355xIndex

    sig = inspect.signature(backend.Mi355xSearcher.search)
    assert "exact" not in sig.parameters and "allowed_ids" not in sig.parameters and "kwargs" in sig.parameters
    src = inspect.getsource(backend.Mi355xSearcher.search)
    assert 'kwargs.get("exact", False)' in src and 'kwargs.get("allowed_ids")' in src
    assert inspect.signature(Mi355xIndex.search_exact).parameters["allowed"].default is None
    assert inspect.signature(Mi355xIndex.search_exact_device).parameters["allowed"].default is None
    assert list(inspect.signature(exact.exact_topk_ip).parameters) == ["Q", "X", "k", "q_block"]
    assert inspect.signature(exact.exact_topk_kernel).parameters["metric"].default == "mips"
