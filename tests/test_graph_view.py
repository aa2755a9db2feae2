"""lm_index_create_view -- an lm_index that searches the graph builder's fixed-capacity level adjacencies in place (csrc/lm_view_impl.h: the
dense-level accessor of k_search_table) -- on the CPU: the product library built for the host (tests/hip_emul/build_emul_lib.py, a thread
per lane) against the unmodified oracle over the CSR the header declares the levels equivalent to (tests/view_ref_util.py) and against
lm_index_search on that CSR.  The scenarios live in tests/emulated_view_cases.py and run in a child process that loads the emulated
library."""
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

    return build_emul_lib.build(tmp_path_factory.mktemp("emul_view"))


def _run(lib, *cases, timeout=3600):
    r = subprocess.run([sys.executable, "-m", "tests.emulated_view_cases", str(lib), *cases], cwd=str(ROOT), capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and "ALL CASES OK" in r.stdout, r.stdout[-3000:] + r.stderr[-5000:]
    assert "MISMATCH" not in r.stdout
    return r.stdout


def test_view_matches_the_oracle_and_the_csr_index(emul_lib):
    out = _run(emul_lib, "view_vs_oracle")
    assert out.count(": ok") == 72  # metric x table dtype x beam x stop rule x (efSearch, k); each line covers both workgroup forms and both max_batch


def test_a_link_to_a_node_the_level_does_not_list(emul_lib):
    _run(emul_lib, "node_absent_from_level")


def test_search_sees_lm_graph_add_links_without_a_new_handle(emul_lib):
    out = _run(emul_lib, "live_after_add_links")
    assert out.count(": ok") == 2


@pytest.mark.parametrize("metric", ["mips", "l2"])
def test_builder_with_view_search_builds_the_csr_search_graph(emul_lib, metric):
    """3000 x 32, M = 8, ef_construction = 40, kernel selector and linker: byte-identical CSR arrays, and no temporary CSR under "view".
    (Minutes in the emulation: every lane of every query's workgroup is an OS thread.)"""
    _run(emul_lib, f"builder_view_equals_csr_{metric}")


def test_rejected_arguments_touch_nothing(emul_lib):
    _run(emul_lib, "argument_checking")


def test_stand_alone_caller_is_clean_under_thread_sanitizer(tmp_path, built_libs):
    """tests/hip_emul/run_view_search.cpp -- a program with its own main over the C ABI -- against the host build of the library, both compiled
    with -fsanitize=thread: in the emulation the kernels' own barriers are the only synchronisation between lanes, so a missing barrier in the
    dense-level accessor (the compaction of an upper-level row, s_pop read by every wave of the level-0 hop) is a reported race.  The program
    compares with an embedded known answer."""
    if not CLANG.exists():
        pytest.skip("needs ROCm's clang++ with the sanitizer runtimes")
    import build_emul_lib

    rt = Path(subprocess.run([str(CLANG), "-print-file-name=libclang_rt.tsan-x86_64.so"], capture_output=True, text=True).stdout.strip())
    if not rt.is_absolute() or not rt.exists():
        pytest.skip("ThreadSanitizer runtime not available")
    lib = build_emul_lib.build(tmp_path, "thread")
    exe = tmp_path / "run_view_search"
    cmd = [str(CLANG), "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=thread", "-shared-libsan", f"-I{ROOT / 'include'}",
           str(ROOT / "tests" / "hip_emul" / "run_view_search.cpp"), str(lib), f"-Wl,-rpath,{lib.parent}", f"-Wl,-rpath,{rt.parent}", "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=1800, env={"TSAN_OPTIONS": "halt_on_error=0"})
    out = r.stdout + r.stderr
    assert "ThreadSanitizer" not in out, out[-4000:]
    assert r.returncode == 0 and "ALL OK" in r.stdout, out[-3000:]


def test_view_search_is_off_by_default():
    """The default path does not change: build_graph_gpu(search="csr"), the backend's gpu_search_view False (the builder is then handed
    search="csr"); the binding lists the new symbol and the ABI revision stays."""
    import inspect

    from leann_amd import _lib, backend
    from leann_amd import gpu_graph_build as gb
    from leann_amd.index import Mi355xIndex

    assert inspect.signature(gb.build_graph_gpu).parameters["search"].default == "csr"
    src = inspect.getsource(backend.Mi355xBuilder._build_graph)
    assert 'bp.get("gpu_search_view", False)' in src and 'search = "view" if' in src
    assert "lm_index_create_view" in _lib.EXPORTED_SYMBOLS and _lib.ABI_REVISION == 6
    assert list(inspect.signature(Mi355xIndex.from_levels).parameters) == ["levels", "ntotal", "d", "metric", "entry_point", "device"]
