"""Insert-step scenarios (lm_graph_insert_batch: one insert batch or refinement step of the batched HNSW builder as one library call) run
against libleann_mi355x_emul.so (tests/hip_emul/build_emul_lib.py: the product's kernels on the CPU, a thread per lane) and the CPU
restatement tests/insert_ref/lm_insert_ref.c.  Imported by tests/test_insert_kernel.py and runnable:
    python -m tests.emulated_insert_cases <path/to/libleann_mi355x_emul.so> <path/to/liblm_insert_ref.so> [case ...]
The scenarios themselves live in tests/insert_ref_util.py (EDGE_CASES), which tests/test_gpu_insert_kernel.py runs on the MI355X over
every (d, metric, table dtype); here scenario number i runs on world number i of those eight (a thread per lane is slow), so that every
width, metric and table type is walked once.  Candidates, candidate distances (as bit patterns), keep masks and the three level arrays are compared byte for byte."""
import sys
from pathlib import Path

import numpy as np

CASES = {}
REF = None
# (d, metric, f16) of scenario number i
WORLDS = [(64, 0, False), (96, 1, True), (64, 1, False), (96, 0, True), (96, 1, False), (64, 0, True), (96, 0, False), (64, 1, True)]


def _load(lib_path: str):
    from leann_amd import _lib

    _lib.LIB_PATH = Path(lib_path)
    _lib._lib = None
    return _lib.load()


def _edge(name):
    def run():
        from tests.insert_ref_util import EDGE_CASES

        w = WORLDS[list(EDGE_CASES).index(name)]
        print(f"d={w[0]} metric={w[1]} f16={w[2]}: " + EDGE_CASES[name](REF, None, *w), flush=True)

    return run


for _name in ("insert_300", "refine_257", "refine_k512", "twin_rows", "overflow", "void_and_duplicates", "alpha", "m_above_candidates"):
    CASES[_name] = _edge(_name)


def case_worlds_cover_everything():
    from tests.insert_ref_util import EDGE_CASES

    assert list(EDGE_CASES) == [c for c in CASES if c in EDGE_CASES] and len(EDGE_CASES) == 8
    assert set(WORLDS) == {(d, m, f) for d in (64, 96) for m in (0, 1) for f in (False, True)}
    print("worlds: ok", flush=True)


CASES["worlds_cover_everything"] = case_worlds_cover_everything


def case_rejections():
    from tests.insert_ref_util import case_rejections as run

    print(run(REF, None), flush=True)


CASES["rejections"] = case_rejections


def case_builder():
    """build_graph_gpu at 320 x 32, M = 8, ef_construction = 40, seed_nodes = 256 (insert batches and refinement both run):
    inserter="kernel" returns the CSR arrays of inserter="torch" byte for byte, and never calls _LevelView.search."""
    import pytest
    import torch

    from leann_amd import gpu_graph_build as gb
    from tests.insert_ref_util import build_both, csr_equal
    from tests.util import clustered

    x = clustered(320, 32, 3, n_centers=12, sigma=0.5)
    for metric in ("mips", "l2"):
        gt, gk, counts = build_both(torch.from_numpy(x), metric, 256)
        gk.validate()
        ok = csr_equal(gt, gk)
        # both phases ran: more insert calls than the refinement alone makes (level 0: ceil(320 / 4096) = 1 step), and refinement did run
        ok = ok and counts["kernel"][0] == 0 and counts["kernel"][1] >= 3 and counts["torch"] == [counts["kernel"][1], 0]
        print(f"builder {metric}: {gk.neighbors.shape[0]} links, {counts['kernel'][1]} insert calls, torch path {counts['torch'][0]} searches: {'ok' if ok else 'MISMATCH'}",
              flush=True)
        assert ok
    for bad in (dict(selector="torch"), dict(linker="torch", search="csr"), dict(search="csr")):
        kw = dict(dict(selector="kernel", linker="kernel", search="view"), **bad)
        with pytest.raises(ValueError):
            gb.build_graph_gpu(torch.from_numpy(x[:50]), "l2", M=4, ef_construction=10, inserter="kernel", **kw)
    with pytest.raises(ValueError):
        gb.build_graph_gpu(torch.from_numpy(x[:50]), "l2", M=4, ef_construction=10, inserter="bogus")


CASES["builder"] = case_builder


if __name__ == "__main__":
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    _load(sys.argv[1])
    from tests.insert_ref_util import load_ref

    REF = load_ref(sys.argv[2])
    import time

    import torch

    torch.set_num_threads(1)
    for name in (sys.argv[3:] or list(CASES)):
        t0 = time.time()
        CASES[name]()
        print(f"[case {name}: {time.time() - t0:.1f} s]", flush=True)
    print("ALL CASES OK")
