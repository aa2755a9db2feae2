"""lm_graph_insert_batch -- one insert batch or refinement step of the batched HNSW builder as one library call on a view index -- on the
CPU: the product library built for the host (tests/hip_emul/build_emul_lib.py, a thread per lane) against tests/insert_ref/lm_insert_ref.c,
an independent C restatement of steps 1 and 3-8 that takes the view search's result as input and ends in the unchanged
tests/select_ref/lm_select_ref.c and tests/link_ref/lm_link_ref.c.  The scenarios live in tests/insert_ref_util.py (shared with
tests/test_gpu_insert_kernel.py) and run in a child process that loads the emulated library (tests/emulated_insert_cases.py): candidates,
candidate distances (bits), keep masks and the three level arrays byte for byte, the builder's opt-in path against its torch path, the
rejections; a stand-alone caller runs under AddressSanitizer."""
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

    from tests.insert_ref_util import compile_ref

    d = tmp_path_factory.mktemp("emul_insert")
    return build_emul_lib.build(d), compile_ref(d)


def _run(libs, *cases, timeout=1800):
    r = subprocess.run([sys.executable, "-m", "tests.emulated_insert_cases", str(libs[0]), str(libs[1]), *cases], cwd=str(ROOT), capture_output=True,
                       text=True, timeout=timeout)
    assert r.returncode == 0 and "ALL CASES OK" in r.stdout, r.stdout[-3000:] + r.stderr[-5000:]
    assert "MISMATCH" not in r.stdout
    return r.stdout


def test_insert_batches_match_the_c_restatement(emul_lib):
    """replace = 0: 300 emptied rows inserted as one batch; m above the number of candidates (the edge slots beyond the kept ones invalid),
    then the same handle without the optional outputs."""
    out = _run(emul_lib, "insert_300", "m_above_candidates", "worlds_cover_everything")
    assert out.count(": ok") == 3


def test_refinement_matches_the_c_restatement(emul_lib):
    """replace = 1: b = 257 at K = 29 and K = 86 with the entry point's, the full, the empty and the out-of-range-slot row."""
    out = _run(emul_lib, "refine_257")
    assert out.count(": ok") == 2


def test_refinement_at_the_largest_k_matches_the_c_restatement(emul_lib):
    """replace = 1: b = 8 at K = 512, the mask's last word and the largest LDS image."""
    out = _run(emul_lib, "refine_k512")
    assert out.count(": ok") == 1


def test_ties_repeats_non_finite_distances_void_and_duplicate_ids(emul_lib):
    """Two identical table rows (position decides; every row dedupes against its stored slots and drops itself -- asserted on the inputs);
    3e38 rows whose distances are not finite reach S and come out empty; void ids and an id listed twice; alpha = 1.2."""
    out = _run(emul_lib, "twin_rows", "overflow", "void_and_duplicates", "alpha")
    assert out.count(": ok") == 1 + 2 + 2 + 1


def test_rejected_arguments_touch_nothing(emul_lib):
    _run(emul_lib, "rejections")


def test_builder_with_the_insert_kernel_builds_the_same_graph(emul_lib):
    """build_graph_gpu at 320 x 32, M = 8, ef_construction = 40, seed_nodes = 256: inserter="kernel" returns the CSR arrays of
    inserter="torch" byte for byte (both with the kernel selector and linker and the view search) and never calls _LevelView.search."""
    out = _run(emul_lib, "builder", timeout=3000)
    assert out.count(": ok") == 2


def test_stand_alone_caller_is_clean_under_address_sanitizer(tmp_path):
    """tests/hip_emul/run_insert.cpp -- a program with its own main over the C ABI -- and the host build of the library, both compiled
    with -fsanitize=address and linked directly (nothing is preloaded).  Several calls on ONE handle with growing and shrinking b and K,
    replace 0 and 1: the index's grow-only buffers serve all of them (the emulated hipMalloc allocates the exact size, so a buffer too small
    for the call that reuses it is a reported overflow, a forgotten one a reported leak); every call equals the same call on a fresh handle."""
    if not CLANG.exists():
        pytest.skip("needs ROCm's clang++ with the sanitizer runtimes")
    import build_emul_lib

    rt = Path(subprocess.run([str(CLANG), "-print-file-name=libclang_rt.asan-x86_64.so"], capture_output=True, text=True).stdout.strip())
    if not rt.is_absolute() or not rt.exists():
        pytest.skip("AddressSanitizer runtime not available")
    lib = build_emul_lib.build(tmp_path, "address")
    exe = tmp_path / "run_insert"
    cmd = [str(CLANG), "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address", "-shared-libsan", f"-I{ROOT / 'include'}",
           str(ROOT / "tests" / "hip_emul" / "run_insert.cpp"), str(lib), f"-Wl,-rpath,{lib.parent}", f"-Wl,-rpath,{rt.parent}", "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=1800, env={"ASAN_OPTIONS": "detect_leaks=1"})
    out = r.stdout + r.stderr
    assert "AddressSanitizer" not in out and "LeakSanitizer" not in out, out[-4000:]
    assert r.returncode == 0 and "ALL OK" in r.stdout, out[-3000:]
    assert "8 calls compared" in r.stdout


def test_insert_kernel_is_off_by_default():
    """The default does not change: build_graph_gpu defaults to inserter="torch", the backend's gpu_insert_kernel to False (the builder is
    then handed no inserter at all); the binding lists the new symbol and the ABI revision stays."""
    import inspect

    from leann_amd import _lib, backend
    from leann_amd import gpu_graph_build as gb
    from leann_amd.index import Mi355xIndex

    assert inspect.signature(gb.build_graph_gpu).parameters["inserter"].default == "torch" and gb.INSERTERS == ("torch", "kernel")
    src = inspect.getsource(backend.Mi355xBuilder._build_graph)
    assert 'bp.get("gpu_insert_kernel", False)' in src and '{"inserter": "kernel"} if insert_kernel else {}' in src
    assert "lm_graph_insert_batch" in _lib.EXPORTED_SYMBOLS and _lib.ABI_REVISION == 6
    assert list(inspect.signature(Mi355xIndex.insert_batch).parameters)[:10] == ["self", "batch", "replace", "kk", "m", "alpha", "params", "adj", "dist", "deg"]
