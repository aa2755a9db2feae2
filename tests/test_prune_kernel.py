"""lm_graph_prune_hubs -- the LEANN paper's high-degree-preserving pruning (Algorithm 3) as HIP kernels -- on the CPU: the product
library built for the host (tests/hip_emul/build_emul_lib.py, a thread per lane) against tests/prune_ref/lm_prune_ref.c, an independent C
restatement of steps 1-5 that ends in the unchanged tests/link_ref/lm_link_ref.c.  The scenarios live in tests/emulated_prune_cases.py and
run in a child process that loads the emulated library: kernel against restatement (adj, dist bits, deg, hubs and indeg byte for byte),
the Python wiring, argument checking; a stand-alone caller runs under ThreadSanitizer."""
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

    from tests.prune_ref_util import compile_ref

    d = tmp_path_factory.mktemp("emul_prune")
    return build_emul_lib.build(d), compile_ref(d)


def _run(libs, *cases, timeout=1800):
    r = subprocess.run([sys.executable, "-m", "tests.emulated_prune_cases", str(libs[0]), str(libs[1]), *cases], cwd=str(ROOT), capture_output=True,
                       text=True, timeout=timeout)
    assert r.returncode == 0 and "ALL CASES OK" in r.stdout, r.stdout[-3000:] + r.stderr[-5000:]
    assert "MISMATCH" not in r.stdout
    return r.stdout


def test_kernel_matches_the_c_restatement(libs):
    out = _run(libs, "kernel_vs_restatement")
    assert out.count(": ok") == 18


def test_empty_graph_and_a_cut_inside_a_group_of_equal_in_degrees(libs):
    out = _run(libs, "empty_graph_and_tie_straddle")
    assert out.count(": ok") == 7


def test_python_wiring_gives_the_restatements_graph(libs):
    _run(libs, "python_wiring")


def test_rejected_arguments_touch_nothing(libs):
    _run(libs, "argument_checking")


def test_stand_alone_caller_is_clean_under_thread_sanitizer(tmp_path, built_libs):
    """tests/hip_emul/run_prune.cpp -- a program with its own main over the C ABI -- against the host build of the library, both compiled
    with -fsanitize=thread: in the emulation the kernels' own barriers are the only synchronisation between lanes, so a missing barrier in
    the histogram, the scan's tile hand-over or the LDS sort steps is a reported race.  The program compares with an embedded known answer."""
    if not CLANG.exists():
        pytest.skip("needs ROCm's clang++ with the sanitizer runtimes")
    import build_emul_lib

    rt = Path(subprocess.run([str(CLANG), "-print-file-name=libclang_rt.tsan-x86_64.so"], capture_output=True, text=True).stdout.strip())
    if not rt.is_absolute() or not rt.exists():
        pytest.skip("ThreadSanitizer runtime not available")
    lib = build_emul_lib.build(tmp_path, "thread")
    exe = tmp_path / "run_prune"
    cmd = [str(CLANG), "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=thread", "-shared-libsan", f"-I{ROOT / 'include'}",
           str(ROOT / "tests" / "hip_emul" / "run_prune.cpp"), str(lib), f"-Wl,-rpath,{lib.parent}", f"-Wl,-rpath,{rt.parent}", "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=1800, env={"TSAN_OPTIONS": "halt_on_error=0"})
    out = r.stdout + r.stderr
    assert "ThreadSanitizer" not in out, out[-4000:]
    assert r.returncode == 0 and "ALL OK" in r.stdout, out[-3000:]


def test_default_pruner_is_the_torch_path(monkeypatch):
    """The default does not change: prune_preserving_hubs defaults to pruner="torch" and return_hubs=False, the backend's gpu_prune_kernel
    to False (the pruning step is then handed no pruner at all; tests/test_gpu_prune_kernel.py runs the parameter end to end).  The binding
    lists both symbols and the ABI revision stays."""
    import inspect

    import numpy as np

    from leann_amd import _lib, backend
    from leann_amd import gpu_graph_build as gb

    sig = inspect.signature(gb.prune_preserving_hubs).parameters
    assert sig["pruner"].default == "torch" and sig["return_hubs"].default is False and gb.PRUNERS == ("torch", "kernel")
    assert list(inspect.signature(gb.prune_level0_kernel).parameters)[:6] == ["table", "adj_int32", "m_low", "n_hubs", "metric", "alpha"]
    assert "lm_graph_prune_hubs" in _lib.EXPORTED_SYMBOLS and "lm_graph_prune_hubs_workspace_bytes" in _lib.EXPORTED_SYMBOLS and _lib.ABI_REVISION == 6
    seen = []
    real = gb.prune_preserving_hubs

    def recording(g, x, M, m_low, hub_fraction=0.02, **kw):
        seen.append(dict(kw))
        return real(g, x, M, m_low, hub_fraction, **kw)

    monkeypatch.setattr(gb, "prune_preserving_hubs", recording)
    data = np.random.default_rng(0).standard_normal((60, 8)).astype(np.float32)
    backend.Mi355xBuilder(M=4, efConstruction=10, hub_preserving_m=2, gpu_build_threshold=10**9)._build_graph(data, "mips").validate()
    assert seen == [{"selector": "torch", "linker": "torch"}]
    src = inspect.getsource(backend.Mi355xBuilder._build_graph)
    assert 'bp.get("gpu_prune_kernel", False)' in src and '{"pruner": "kernel"} if prune_kernel else {}' in src
