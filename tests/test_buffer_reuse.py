"""The host-pointer entry points share the index's grow-only device buffers (csrc/lm_devbuf.h: query / result staging, the padded queries, the
uploaded allow-list, the per-query counters, the workspaces).  tests/hip_emul/run_buffer_reuse.cpp -- a program with its own main over the
C ABI -- calls all of them in turn on one index, with n going 1, 5, 2, 9 and k 3, 10, and compares every result with a fresh index's."""
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CLANG = Path("/opt/rocm/lib/llvm/bin/clang++")
sys.path.insert(0, str(ROOT / "tests" / "hip_emul"))


def test_stand_alone_caller_is_clean_under_address_sanitizer_and_leaves_no_leak(tmp_path):
    """The program and the host build of the library, both compiled with -fsanitize=address and linked directly (nothing is preloaded).  The
    emulated hipMalloc allocates the exact size, so a shared buffer too small for the call that reuses it is a reported overflow; leak
    detection is on, so a device buffer that lm_index_free (the index's destructor-owned buffers) does not free is a reported leak."""
    if not CLANG.exists():
        pytest.skip("needs ROCm's clang++ with the sanitizer runtimes")
    import build_emul_lib

    rt = Path(subprocess.run([str(CLANG), "-print-file-name=libclang_rt.asan-x86_64.so"], capture_output=True, text=True).stdout.strip())
    if not rt.is_absolute() or not rt.exists():
        pytest.skip("AddressSanitizer runtime not available")
    lib = build_emul_lib.build(tmp_path, "address")
    exe = tmp_path / "run_buffer_reuse"
    cmd = [str(CLANG), "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address", "-shared-libsan", f"-I{ROOT / 'include'}",
           str(ROOT / "tests" / "hip_emul" / "run_buffer_reuse.cpp"), str(lib), f"-Wl,-rpath,{lib.parent}", f"-Wl,-rpath,{rt.parent}", "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=1800, env={"ASAN_OPTIONS": "detect_leaks=1"})
    out = r.stdout + r.stderr
    assert "AddressSanitizer" not in out and "LeakSanitizer" not in out, out[-4000:]
    assert r.returncode == 0 and "ALL OK" in r.stdout, out[-3000:]
    assert "89 calls compared" in r.stdout  # 2 x 4 x 10 on the CSR index, the hub cache, 2 x 4 on the view
