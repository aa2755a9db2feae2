"""The graph search's edge cases (tests/emulated_graph_search_cases.py) on the CPU: the product library built for the host
(tests/hip_emul/build_emul_lib.py, a thread per lane) against oracle/lm_oracle.c -- labels, distance bits, ndis / nexpand / nrounds and the
provider's request list of every round.  The premises of every case (what its inputs must make the kernels do) are asserted here from the
inputs and the oracle alone, without the library; the scenarios run in a child process that loads the emulated library.
tests/test_gpu_graph_search_edges.py runs the same scenarios on the MI355X, at full size and in every world."""
import os
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
    return build_emul_lib.build(tmp_path_factory.mktemp("emul_graph_search"))


@pytest.fixture(scope="module")
def oracle_lib(built_libs):
    from oracle import oracle as orc

    return orc.lib()


def _run(lib, *names, timeout=800, env=None):
    r = subprocess.run([sys.executable, "-m", "tests.emulated_graph_search_cases", str(lib), *names], cwd=str(ROOT), capture_output=True, text=True,
                       timeout=timeout, env=None if env is None else dict(os.environ, **env))
    assert r.returncode == 0 and "ALL CASES OK" in r.stdout, r.stdout[-3000:] + r.stderr[-5000:]
    return r.stdout


def test_forms_cover_every_instantiation():
    """Case A's list of forms against the launchers' source: every CASE label of launch_update_nch and launch_persist_nch, every (MODE, NT) /
    NT value their macros instantiate and every (L2, F16) pair has a form, and the list names nothing the source lacks.  A list that lost a
    width is caught."""
    from tests.emulated_graph_search_cases import assert_forms_cover_every_instantiation, forms

    assert_forms_cover_every_instantiation()
    assert len(forms()) == 9 * 2 * (2 * 4 + 4)
    with pytest.raises(AssertionError, match="instantiations without a form"):
        assert_forms_cover_every_instantiation([f for f in forms() if f[1] != 5])


def test_merge_premises(oracle_lib):
    """Case B's hub chain makes the level-0 rounds of a one-query search evaluate exactly the designed numbers of new nodes, and those fall
    on both sides of rank_merge_unsorted_pays at 64 and at 256 threads: a first hop of 301, the largest counting n and the next one with the
    pool full, powers of two and 2^m + 1 on the sorting side."""
    from tests.emulated_graph_search_cases import assert_merge_premises

    ns, npool0 = assert_merge_premises()
    assert ns[:7] == [301, 256, 257, 160, 161, 85, 86] and npool0[:2] == [1, 96]


def test_expansion_edge_premises(oracle_lib):
    """Case C's graphs make some round pop 64, 65 and 130 nodes (a partial p0 pass), empty lists between non-empty ones, lists longer than
    64 and 256, more than 256 slots with fewer fresh nodes, duplicate ids inside and across lists, self loops, a walk seeded at an entry
    point without neighbours, both stop rules biting, and NaN / +-inf / -0 rows evaluated under both metrics and by the zero query."""
    from tests.emulated_graph_search_cases import assert_edge_premises

    assert_edge_premises()


def test_dedup_tile_premises(oracle_lib):
    """Case E's graph makes a round ask for ids in all three tiles of the request bitmap and in its last partial word."""
    from tests.emulated_graph_search_cases import assert_tiles_premises, tiles_world

    assert_tiles_premises(tiles_world())


@pytest.mark.parametrize("nch", [1, 2, 3, 4, 5, 6, 8, 12, 16])
def test_every_form_the_launchers_can_reach(emul_lib, nch):
    """Case A at one padded width: both metrics, fp32 and fp16 rows through the persistent and the lock-step kernels at 256 and 64 threads,
    and the three row-addressing modes of k_update (rank at both widths, rank with identity, memo slot); d = 64 nch - 3 and every 64-wide
    chunk changes the oracle's labels (asserted)."""
    assert f"forms width {64 * nch}: ok" in _run(emul_lib, f"every_form:{nch}")


def test_both_merge_branches_at_both_widths(emul_lib):
    """Case B at the library's own limit (the hub chain reaches both branches by construction) and with the emulation's limit moved to 0
    (every round sorts) and to 12."""
    _run(emul_lib, "merge_branches")
    for limit in ("0", "12"):
        _run(emul_lib, "merge_branches", env={"LM_EMUL_COUNTING_MERGE_LIMIT": limit})


def test_expansion_edges(emul_lib):
    """Case C: each scenario in two worlds, all eight worlds walked across the scenarios (asserted in the case)."""
    from tests.emulated_graph_search_cases import EDGE_SHAPES

    assert _run(emul_lib, "expansion_edges").count(": ok") == 2 * len(EDGE_SHAPES)


def test_lds_envelope_of_a_csr_index(emul_lib):
    """Case D: the largest efSearch of either kernel is exact (the persistent one also equals brute force over the reachable set), the next is
    LM_EINVAL naming the LDS with the outputs untouched; between the limits the table is served and the provider refused."""
    _run(emul_lib, "lds_envelope")


def test_dedup_over_several_tiles(emul_lib):
    """Case E at its full N = 262181 (the host build takes about 10 s for it): rank addressing and memo, then the hub cache on the tile
    borders.  The wave form and the identity path of this case run on the GPU only."""
    _run(emul_lib, "dedup_tiles")


def test_overflowing_sizes_are_refused_before_anything_is_allocated(emul_lib):
    """Case F: batch_size 2^31 - 1 and 1 000 000, beam_size 2^31 - 1 and one whose product with the largest degree passes 2^31 are LM_EINVAL
    with the outputs untouched and the handle usable; the largest batch_size that fits and the one below equal the oracle."""
    _run(emul_lib, "overflow_refusals")
