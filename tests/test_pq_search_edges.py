"""The DiskANN-style search's edge cases (tests/emulated_pq_search_cases.py) on the CPU: the product library built for the host
(tests/hip_emul/build_emul_lib.py, a thread per lane, 256 threads per query) against oracle/lm_oracle_pq.c and
oracle/lm_oracle_diskann.c -- labels, distance bits and counts.  The scenarios run in a child process that loads the emulated library;
tests/test_gpu_pq_search_edges.py runs the same lists on the MI355X at full size and all three workgroup widths."""
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

    from oracle import oracle as orc

    orc.lib()
    return build_emul_lib.build(tmp_path_factory.mktemp("emul_pq_search"))


def _run(lib, *names, timeout=1800):
    r = subprocess.run([sys.executable, "-m", "tests.emulated_pq_search_cases", str(lib), *names], cwd=str(ROOT), capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0 and "ALL CASES OK" in r.stdout, r.stdout[-3000:] + r.stderr[-5000:]
    return r.stdout


def test_layouts_cover_every_instantiation():
    """Case A's list against the kernel source: every label of adc1's switch, both generic loops, a table shorter than one group of
    entries, all nine k_pq_rerank widths, an empty chunk, a remainder of the 4-unrolled loop, mixed lengths among a thread's four
    entries at every workgroup width."""
    from tests.emulated_pq_search_cases import assert_layouts_cover_every_instantiation

    assert_layouts_cover_every_instantiation()


def test_degenerate_graph_premises():
    from tests.emulated_pq_search_cases import assert_degenerate_premises, degenerate_inputs

    assert_degenerate_premises(degenerate_inputs())


def test_every_adc_lut_and_rerank_instantiation(emul_lib):
    from tests.emulated_pq_search_cases import LAYOUTS

    assert _run(emul_lib, "every_instantiation").count(": ok") == len(LAYOUTS)


def test_degenerate_graphs_ties_and_special_values(emul_lib):
    _run(emul_lib, "degenerate_graphs", "ties_and_special_values")


def test_wide_hops_and_the_lds_envelope(emul_lib):
    _run(emul_lib, "wide_hops", "lds_envelope")


def test_expanded_set_overflow_falls_back_to_the_final_list(emul_lib):
    assert _run(emul_lib, "expanded_overflow").count("queries over the cap: ok") == 5
