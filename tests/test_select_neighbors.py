"""lm_select_neighbors -- the select-neighbours heuristic of graph construction as a HIP kernel -- on the CPU: the product library built
for the host (tests/hip_emul/build_emul_lib.py, a thread per lane) against tests/select_ref/lm_select_ref.c, an independent C
restatement whose distance function is the oracle's orc_dist.  The scenarios live in tests/emulated_select_cases.py and run in a child
process that loads the emulated library: kernel against restatement (byte-equal keep masks), three-way agreement with the builder's
torch form where the arithmetic is exact, the builder's `selector` wiring, argument checking."""
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

    from tests.select_ref_util import compile_ref

    d = tmp_path_factory.mktemp("emul_select")
    return build_emul_lib.build(d), compile_ref(d)


def _run(libs, *cases, timeout=1800):
    r = subprocess.run([sys.executable, "-m", "tests.emulated_select_cases", str(libs[0]), str(libs[1]), *cases], cwd=str(ROOT), capture_output=True,
                       text=True, timeout=timeout)
    assert r.returncode == 0 and "ALL CASES OK" in r.stdout, r.stdout[-3000:] + r.stderr[-5000:]
    assert "MISMATCH" not in r.stdout
    return r.stdout


def test_kernel_matches_the_c_restatement(libs):
    out = _run(libs, "kernel_vs_restatement")
    assert out.count(": ok") >= 40


def test_torch_scan_restatement_and_kernel_agree_on_exact_arithmetic(libs):
    _run(libs, "three_way_on_exact_arithmetic")


def test_builder_and_pruning_give_the_same_graph_with_either_selector(libs):
    _run(libs, "builder_wiring")


def test_rejected_arguments_and_unknown_selector(libs):
    _run(libs, "argument_checking")


def test_default_selector_is_the_torch_path():
    """The default does not change: build_graph_gpu / prune_preserving_hubs / _LevelGraph default to selector="torch", the backend's
    gpu_select_kernel to False."""
    import inspect

    from leann_amd import gpu_graph_build as gb

    for f in (gb.build_graph_gpu, gb.prune_preserving_hubs, gb._LevelGraph.__init__):
        assert inspect.signature(f).parameters["selector"].default == "torch"
    assert gb._selector_fn("torch") is gb._select_heuristic and gb._selector_fn("kernel") is gb.select_neighbors_kernel
