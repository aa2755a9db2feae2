"""lm_pq_scan / lm_pq_flat_search -- the flat PQ scan with an allow-list and the PQ path's rerank tail, as HIP kernels -- on the CPU: the product
library built for the host (tests/hip_emul/build_emul_lib.py, a thread per lane) against the reference composed in tests/pq_flat_ref_util.py
from the oracle's lookup table, ADC sum, key order and orc_dist; labels equal, distance bits equal.  The scenarios live in
tests/emulated_pq_flat_cases.py and run in a child process that loads the emulated library."""
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

    return build_emul_lib.build(tmp_path_factory.mktemp("emul_pq_flat"))


def _run(lib, *cases, timeout=1800):
    r = subprocess.run([sys.executable, "-m", "tests.emulated_pq_flat_cases", str(lib), *cases], cwd=str(ROOT), capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and "ALL CASES OK" in r.stdout, r.stdout[-3000:] + r.stderr[-5000:]
    assert "MISMATCH" not in r.stdout
    return r.stdout


def test_scan_matches_the_reference_in_every_slicing_regime(emul_lib):
    out = _run(emul_lib, "slicing")
    assert out.count(": ok") >= 8


def test_table_layouts_metrics_and_query_stride(emul_lib):
    _run(emul_lib, "layouts")


def test_ties_across_slices_nan_zero_and_short_arrays(emul_lib):
    _run(emul_lib, "ranking")


def test_allow_list_matches_the_reference_on_the_compacted_codes(emul_lib):
    _run(emul_lib, "allow_list")


def test_rejected_arguments_touch_nothing(emul_lib):
    _run(emul_lib, "argument_checking")


def test_index_form_provider_tables_stats_and_exact_cross_check(emul_lib):
    _run(emul_lib, "index")


def test_index_form_rejections_leave_the_outputs_untouched(emul_lib):
    _run(emul_lib, "index_rejections")


def test_batch_search_is_what_it_was_before_the_tail_was_shared(emul_lib):
    """lm_pq_batch_search on the fixed small index of tests/emulated_pq_flat_cases.py: labels, distance bits and (ndis, nexpand, nrounds,
    nunique) as recorded at the parent commit (BATCH_SEARCH_AT_PARENT: first labels row [125, 153, 191, 81, 58], stats [343, 76, 13, 23]
    through the provider and [343, 76, 13, 0] through the table)."""
    _run(emul_lib, "batch_search_unchanged")


def test_scan_wrapper_and_backend_wiring(emul_lib):
    _run(emul_lib, "wiring")


def test_pq_flat_is_off_by_default():
    """The default paths do not change: both searchers take `pq_flat` / `allowed_ids` through **kwargs only (absent = off), the literals the
    exact search's test reads stay, the index methods' allow-list defaults to None."""
    import inspect

    from leann_amd import backend, pq
    from leann_amd.index import Mi355xIndex

    for cls in (backend.Mi355xSearcher, backend.Mi355xDiskannSearcher):
        sig = inspect.signature(cls.search)
        assert "pq_flat" not in sig.parameters and "allowed_ids" not in sig.parameters and "kwargs" in sig.parameters
        assert 'kwargs.get("pq_flat", False)' in inspect.getsource(cls.search)
    src = inspect.getsource(backend.Mi355xSearcher.search)
    assert 'kwargs.get("exact", False)' in src and 'kwargs.get("allowed_ids")' in src
    assert inspect.signature(Mi355xIndex.pq_flat_search).parameters["allowed"].default is None
    assert inspect.signature(Mi355xIndex.pq_flat_search_device).parameters["allowed"].default is None
    assert inspect.signature(pq.pq_scan_kernel).parameters["allowed"].default is None
