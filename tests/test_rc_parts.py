"""The recompute provider's part planner (leann_amd/csrc/lm_rc_parts.h) as a stand-alone host program under AddressSanitizer and
UndefinedBehaviorSanitizer: hand-made cumulative lengths -> split points -> part ranges (no GPU, no library, nothing loaded into Python).
Built with the ROCm toolchain's clang++, as the other sanitizer programs of this suite are."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CLANG = Path("/opt/rocm/lib/llvm/bin/clang++")


def test_part_planner_standalone_sanitized(tmp_path):
    exe = tmp_path / "rc_parts_check"
    src = ROOT / "tests" / "rc_parts" / "rc_parts_check.cpp"
    r = subprocess.run([str(CLANG), "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-o", str(exe), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env={"ASAN_OPTIONS": "detect_leaks=1"})
    assert r.returncode == 0, r.stdout + r.stderr
    assert "RC-PARTS-OK" in r.stdout
