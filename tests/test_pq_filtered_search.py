"""lm_pq_batch_search_filtered -- the DiskANN-style traversal with an allow-list (csrc/lm_pq_impl.h: k_pq_traverse<NTH, true>) -- on the CPU:
the product library built for the host (tests/hip_emul/build_emul_lib.py, a thread per lane) against the reference composed from the
unmodified oracle in tests/pq_filtered_ref_util.py; labels, distance bits, stats, request lists and "filtered_allowed_evals" equal.  The
scenarios live in tests/emulated_pq_filtered_cases.py and run in a child process that loads the emulated library."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
CLANG = Path("/opt/rocm/lib/llvm/bin/clang++")
sys.path.insert(0, str(ROOT / "tests" / "hip_emul"))


@pytest.fixture(scope="module")
def emul_lib(tmp_path_factory, built_libs):
    if not CLANG.exists():
        pytest.skip("needs ROCm's clang++ as a host compiler")
    import build_emul_lib

    return build_emul_lib.build(tmp_path_factory.mktemp("emul_pq_filtered"))


def _run(lib, *cases, timeout=1800):
    r = subprocess.run([sys.executable, "-m", "tests.emulated_pq_filtered_cases", str(lib), *cases], cwd=str(ROOT), capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and "ALL CASES OK" in r.stdout, r.stdout[-3000:] + r.stderr[-5000:]
    assert "MISMATCH" not in r.stdout
    return r.stdout


def test_modes_and_allow_lists(emul_lib):
    out = _run(emul_lib, "modes_and_allow_lists")
    assert out.count(": ok") >= 3 * 2 * 4 * 9


def test_the_collecting_threshold_is_the_allowed_lists_own(emul_lib):
    _run(emul_lib, "collecting_threshold")


def test_staging_overflow_takes_several_rounds(emul_lib):
    _run(emul_lib, "staging_overflow")


def test_degenerate_graphs(emul_lib):
    _run(emul_lib, "degenerate_graphs")


def test_ranking_ties_nan_and_the_zero_query(emul_lib):
    _run(emul_lib, "ranking")


def test_invariants_alone_and_together_entries_calls_in_a_row_and_the_shared_workspace(emul_lib):
    _run(emul_lib, "invariants")


def test_lds_envelope_largest_l_and_the_next_refused(emul_lib):
    _run(emul_lib, "lds_envelope")


def test_rejected_arguments_touch_nothing(emul_lib):
    _run(emul_lib, "rejections")


def test_index_wrappers_and_backend_wiring(emul_lib):
    _run(emul_lib, "wiring")


def test_stand_alone_caller_is_clean_under_thread_sanitizer(tmp_path, built_libs):
    """tests/hip_emul/run_pq_filtered_search.cpp -- a program with its own main over the C ABI -- against the host build of the library, both
    compiled with -fsanitize=thread: in the emulation the kernel's own barriers are the only synchronisation between lanes, so a missing
    barrier round the allowed-only list, its staging area or the merge output it shares with the walk is a reported race.  It runs the
    collecting-threshold and the staging-overflow shapes at 256 lanes per query."""
    if not CLANG.exists():
        pytest.skip("needs ROCm's clang++ with the sanitizer runtimes")
    import build_emul_lib

    rt = Path(subprocess.run([str(CLANG), "-print-file-name=libclang_rt.tsan-x86_64.so"], capture_output=True, text=True).stdout.strip())
    if not rt.is_absolute() or not rt.exists():
        pytest.skip("ThreadSanitizer runtime not available")
    lib = build_emul_lib.build(tmp_path, "thread")
    exe = tmp_path / "run_pq_filtered_search"
    cmd = [str(CLANG), "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=thread", "-shared-libsan", f"-I{ROOT / 'include'}",
           str(ROOT / "tests" / "hip_emul" / "run_pq_filtered_search.cpp"), str(lib), f"-Wl,-rpath,{lib.parent}", f"-Wl,-rpath,{rt.parent}", "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=1800, env={"TSAN_OPTIONS": "halt_on_error=0"})
    out = r.stdout + r.stderr
    assert "ThreadSanitizer" not in out, out[-4000:]
    assert r.returncode == 0 and "ALL OK" in r.stdout, out[-3000:]


def test_the_reference_has_the_premises_the_cases_rely_on():
    """On the reference alone, at the cases' draw (default_rng(7): 50 %, 10 %, 2 % in this order), for case A's m16-d64 and m96-d384 inputs at
    n = 200 and n = 600, both metrics, 9 queries, k = 10, L = 40, W = 4: the 10 % list gives k hits for every query although post-filtering
    the oracle's final list gives fewer than k for every query, and the 2 % list gives fewer than k for every query -- so the cases are not
    ones that post-filtering the unfiltered kernel's result would pass."""
    from oracle import oracle as orc
    from tests import emulated_pq_filtered_cases as cases
    from tests import emulated_pq_search_cases as pc
    from tests import pq_filtered_ref_util as pr

    orc.lib()
    k, L, W = 10, 40, 4
    for name in ("m16-d64", "m96-d384"):
        for emulated in (True, False):
            for metric in (pr.IP, pr.L2):
                x, g, q, cb, codes, off = pc._layout_inputs(cases.layout(name), metric, emulated)
                assert x.shape[0] == (200 if emulated else 600) and q.shape[0] == 9
                R = pr.Reference(g, cb, codes, off)
                _, m10, m2 = cases.draws(x.shape[0])
                for i in range(9):
                    q1 = np.ascontiguousarray(q[i])
                    assert len(R.flist(q1, k, L, W, m10)[0]) >= k, (name, emulated, metric, i)
                    assert len(R.post_filter_hits(q1, k, L, W, m10)) < k, (name, emulated, metric, i)
                    assert len(R.flist(q1, k, L, W, m2)[0]) < k, (name, emulated, metric, i)


def test_the_filtered_traversal_is_off_by_default():
    """The default path does not change: Mi355xDiskannSearcher.search takes `graph_filter` through **kwargs only (absent = off),
    pq_search_filtered's allow-list defaults to None, pq_search keeps its signature, the ABI revision stays."""
    import inspect

    from leann_amd import _lib, backend
    from leann_amd.index import Mi355xIndex

    sig = inspect.signature(backend.Mi355xDiskannSearcher.search)
    assert "graph_filter" not in sig.parameters and "allowed_ids" not in sig.parameters and "kwargs" in sig.parameters
    assert 'kwargs.get("graph_filter", False)' in inspect.getsource(backend.Mi355xDiskannSearcher.search)
    assert inspect.signature(Mi355xIndex.pq_search_filtered).parameters["allowed"].default is None
    assert inspect.signature(Mi355xIndex.pq_search_filtered_device).parameters["allowed"].default is None
    assert list(inspect.signature(Mi355xIndex.pq_search).parameters) == ["self", "queries", "k", "params"]
    assert "lm_pq_batch_search_filtered" in _lib.EXPORTED_SYMBOLS and "lm_pq_batch_search_filtered_device" in _lib.EXPORTED_SYMBOLS
    assert _lib.ABI_REVISION == 6
