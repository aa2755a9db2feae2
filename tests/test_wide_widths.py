"""The wide padded widths (csrc/lm_wide_impl.h) on the CPU: the product library built for the host (tests/hip_emul/build_emul_lib.py, a thread per
lane) at 1536 and 4096 against the oracle.  The scenarios live in tests/emulated_wide_cases.py and run in a child process."""
import subprocess
import sys

from tests.test_exact_search import ROOT, emul_lib  # noqa: F401  (the fixture that builds the emulated library)


def test_wide_widths_match_the_oracle(emul_lib):  # noqa: F811
    r = subprocess.run([sys.executable, "-m", "tests.emulated_wide_cases", str(emul_lib)], cwd=str(ROOT), capture_output=True, text=True, timeout=850)
    assert r.returncode == 0 and "ALL CASES OK" in r.stdout, r.stdout[-3000:] + r.stderr[-5000:]
