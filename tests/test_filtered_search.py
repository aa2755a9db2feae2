"""lm_index_search_filtered -- the HNSW graph search with an allow-list (csrc/lm_filter_impl.h: k_filter_collect) -- on the CPU: the product
library built for the host (tests/hip_emul/build_emul_lib.py, a thread per lane) against the reference composed from the unmodified oracle in
tests/filtered_ref_util.py; labels, distance bits, stats, request lists and "filtered_allowed_evals" equal.  The scenarios live in
tests/emulated_filtered_cases.py and run in a child process that loads the emulated library."""
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

    return build_emul_lib.build(tmp_path_factory.mktemp("emul_filtered"))


def _run(lib, *cases, timeout=1800):
    r = subprocess.run([sys.executable, "-m", "tests.emulated_filtered_cases", str(lib), *cases], cwd=str(ROOT), capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and "ALL CASES OK" in r.stdout, r.stdout[-3000:] + r.stderr[-5000:]
    assert "MISMATCH" not in r.stdout
    return r.stdout


def test_every_source_provider_memo_hub_cache_and_tables(emul_lib):
    out = _run(emul_lib, "sources")
    assert out.count(": ok") >= 20


def test_parameters_k_above_efsearch_and_more_allowed_keys_than_k(emul_lib):
    _run(emul_lib, "parameters")


def test_allow_lists(emul_lib):
    _run(emul_lib, "allow_lists")


def test_ranking_ties_nan_zero_query_and_a_seed_without_neighbours(emul_lib):
    _run(emul_lib, "ranking")


def test_invariants_batch_cuts_entries_and_no_state_between_calls(emul_lib):
    _run(emul_lib, "invariants")


def test_rejected_arguments_touch_nothing(emul_lib):
    _run(emul_lib, "rejections")


def test_index_wrappers_and_backend_wiring(emul_lib):
    _run(emul_lib, "wiring")


def test_stand_alone_caller_is_clean_under_thread_sanitizer(tmp_path, built_libs):
    """tests/hip_emul/run_filtered_search.cpp -- a program with its own main over the C ABI -- against the host build of the library, both
    compiled with -fsanitize=thread: in the emulation the kernels' own barriers are the only synchronisation between lanes, so a missing barrier
    in k_filter_collect, or a write of it into anything the walk reads, is a reported race."""
    if not CLANG.exists():
        pytest.skip("needs ROCm's clang++ with the sanitizer runtimes")
    import build_emul_lib

    rt = Path(subprocess.run([str(CLANG), "-print-file-name=libclang_rt.tsan-x86_64.so"], capture_output=True, text=True).stdout.strip())
    if not rt.is_absolute() or not rt.exists():
        pytest.skip("ThreadSanitizer runtime not available")
    lib = build_emul_lib.build(tmp_path, "thread")
    exe = tmp_path / "run_filtered_search"
    cmd = [str(CLANG), "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=thread", "-shared-libsan", f"-I{ROOT / 'include'}",
           str(ROOT / "tests" / "hip_emul" / "run_filtered_search.cpp"), str(lib), f"-Wl,-rpath,{lib.parent}", f"-Wl,-rpath,{rt.parent}", "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=1800, env={"TSAN_OPTIONS": "halt_on_error=0"})
    out = r.stdout + r.stderr
    assert "ThreadSanitizer" not in out, out[-4000:]
    assert r.returncode == 0 and "ALL OK" in r.stdout, out[-3000:]


def test_the_reference_has_the_premises_the_cases_rely_on():
    """On the reference alone: at the cases' draw the 50 % list gives k hits for every query and the 2 % list fewer than k for at least one."""
    import numpy as np

    from tests import emulated_filtered_cases as cases

    for name in ("ip64", "l2_100"):
        W = cases.world(name)
        q = W.queries(8, 79)
        rng = np.random.default_rng(cases.DRAW_SEED[name])
        m50, m2 = rng.random(W.n) < 0.5, rng.random(W.n) < 0.02
        assert (W.R.expected(q, 10, m50, 64)[3] == 10).all()
        assert (W.R.expected(q, 10, m2, 64)[3] < 10).any()


def test_graph_filter_is_off_by_default():
    """The default path does not change: Mi355xSearcher.search takes `graph_filter` through **kwargs only (absent = off), search_filtered's
    allow-list defaults to None, search keeps its signature."""
    import inspect

    from leann_amd import _lib, backend
    from leann_amd.index import Mi355xIndex

    sig = inspect.signature(backend.Mi355xSearcher.search)
    assert "graph_filter" not in sig.parameters and "allowed_ids" not in sig.parameters and "kwargs" in sig.parameters
    src = inspect.getsource(backend.Mi355xSearcher.search)
    assert 'kwargs.get("graph_filter", False)' in src and 'kwargs.get("allowed_ids")' in src
    assert inspect.signature(Mi355xIndex.search_filtered).parameters["allowed"].default is None
    assert inspect.signature(Mi355xIndex.search_filtered_device).parameters["allowed"].default is None
    assert list(inspect.signature(Mi355xIndex.search).parameters) == ["self", "queries", "k", "params"]
    assert "lm_index_search_filtered" in _lib.EXPORTED_SYMBOLS and "lm_index_search_filtered_device" in _lib.EXPORTED_SYMBOLS
    assert _lib.ABI_REVISION == 6
