"""CSR-assembly scenarios run against libleann_mi355x_emul.so (tests/hip_emul/build_emul_lib.py: the product's kernels on the CPU, a
thread per lane).  Imported by tests/test_csr_kernel.py and runnable:
    python -m tests.emulated_csr_cases <path/to/libleann_mi355x_emul.so> [case ...]"""
import sys
from pathlib import Path

import numpy as np

CASES = {}


def case_kernel_vs_reference():
    """Every ntotal at the 16-lane form, the other two forms where the thread-per-lane emulation stays quick."""
    from tests.csr_ref_util import NTOTALS, check_case

    for n, cap in [(n, 4) for n in NTOTALS] + [(0, 64), (1, 96), (1025, 64), (1025, 96)]:
        check_case("cpu", n, cap)
        print(f"csr n={n} cap={cap}: ok", flush=True)


CASES["kernel_vs_reference"] = case_kernel_vs_reference


def case_rejections():
    """Every argument the header rejects is LM_EINVAL and launches nothing (the outputs keep their fill); ntotal == 0 and n_rows == 0 are
    fine; the workspace function is 0 for what the calls reject."""
    import ctypes as C

    from leann_amd import _lib

    lib = _lib.load()
    n, cap, fill = 6, 4, 0x6E
    adj, up_nodes, up_adj = np.full((n, cap), -1, np.int32), np.array([1, 4], np.int32), np.full((2, cap), -1, np.int32)
    lv0 = dict(nodes0=None, adj0=adj.ctypes.data, rows0=n, cap0=cap, nodes1=up_nodes.ctypes.data, adj1=up_adj.ctypes.data, rows1=2, cap1=cap)

    def levels(**over):
        a = dict(lv0, **over)
        return (_lib.GraphLevel * 2)(*(_lib.GraphLevel(a["nodes" + i], a["adj" + i], a["rows" + i], a["cap" + i]) for i in "01"))

    need = int(lib.lm_graph_levels_to_csr_workspace_bytes(n, levels(), 2))
    assert need > 0
    ws = np.zeros(need + 8, np.uint8)
    outs = {k: np.full(64, fill, np.uint8) for k in ("lv", "no", "lp", "nb", "adj", "deg")}
    ptr = {k: o.ctypes.data for k, o in outs.items()}
    nptr, nnb = C.c_int64(-5), C.c_int64(-5)

    def fwd(which, **over):  # which: c = _count, f = _fill, w = the workspace function
        a = dict(dict(ptr, n=n, arr=levels(**{k: v for k, v in over.items() if k in lv0}), nl=2, ws=ws.ctypes.data, wsb=need, p1=C.byref(nptr), p2=C.byref(nnb)), **over)
        calls = dict(c=lambda: lib.lm_graph_levels_to_csr_count(a["n"], a["arr"], a["nl"], a["lv"], a["no"], a["ws"], a["wsb"], a["p1"], a["p2"], None),
                     f=lambda: lib.lm_graph_levels_to_csr_fill(a["n"], a["arr"], a["nl"], a["lv"], a["no"], a["lp"], a["nb"], a["ws"], a["wsb"], None),
                     w=lambda: lib.lm_graph_levels_to_csr_workspace_bytes(a["n"], a["arr"], a["nl"]))
        return {w: calls[w]() for w in which}

    def untouched():
        return all((o == fill).all() for o in outs.values()) and nptr.value == -5 and nnb.value == -5

    bad = [("cfw", dict(arr=None)), ("cfw", dict(nl=0)), ("cfw", dict(nl=_lib.CSR_MAX_LEVELS + 1)), ("cfw", dict(n=-1)), ("cfw", dict(n=1 << 31)), ("cfw", dict(nodes0=up_nodes.ctypes.data)),
           ("cfw", dict(rows0=n - 1)), ("cfw", dict(cap0=0)), ("cfw", dict(cap1=-1)), ("cfw", dict(rows1=-1)), ("cfw", dict(rows1=n + 1)), ("cfw", dict(nodes1=None)),
           ("cfw", dict(adj0=None)), ("cfw", dict(adj1=None)), ("c", dict(lv=None)), ("c", dict(no=None)), ("c", dict(p1=None)), ("c", dict(p2=None)), ("f", dict(lv=None)),
           ("f", dict(no=None)), ("f", dict(lp=None)), ("f", dict(nb=None)), ("cf", dict(ws=None)), ("cf", dict(ws=ws.ctypes.data + 4)), ("cf", dict(wsb=need - 1)), ("cf", dict(wsb=0))]
    for which, over in bad:
        rc = fwd(which, **over)
        assert all(rc[w] == (0 if w == "w" else _lib.LM_EINVAL) for w in which) and untouched(), (over, rc)

    def back(**over):
        a = dict(dict(n=n, no=ws.ctypes.data, lp=ws.ctypes.data, nlp=2, nb=ws.ctypes.data, nnb=1, lv=ws.ctypes.data, level=0, nodes=None, rows=n, cap=cap, adj=ptr["adj"], deg=ptr["deg"]),
                 **over)
        return lib.lm_graph_csr_to_level(a["n"], a["no"], a["lp"], a["nlp"], a["nb"], a["nnb"], a["lv"], a["level"], a["nodes"], a["rows"], a["cap"], a["adj"], a["deg"], None, None)

    for over in (dict(n=-1), dict(n=1 << 31), dict(nlp=-1), dict(nnb=-1), dict(level=-1), dict(cap=0), dict(rows=-1), dict(rows=n + 1), dict(rows=2), dict(no=None),
                 dict(lv=None), dict(adj=None), dict(lp=None), dict(nb=None)):
        assert back(**over) == _lib.LM_EINVAL and untouched(), over
    assert back(nodes=up_nodes.ctypes.data, rows=0) == 0 and back(n=0, rows=0, no=None, lv=None, adj=None) == 0 and untouched()
    # ntotal == 0: LM_OK without a workspace, the sizes are 0 and node_offsets[0] = 0 is the only thing written
    rc = fwd("cfw", n=0, rows0=0, rows1=0, adj0=None, adj1=None, nodes1=None, ws=None, wsb=0, lv=None)
    assert rc == dict(c=0, f=0, w=0) and nptr.value == 0 and nnb.value == 0 and (outs["no"][:8] == 0).all() and (outs["no"][8:] == fill).all()
    print("rejections: ok", flush=True)


CASES["rejections"] = case_rejections


def case_builder_wiring():
    """build_graph_gpu at 320 x 32, M = 8 on the view path: assembler="kernel" returns the arrays of assembler="numpy" byte for byte; so does
    prune_preserving_hubs(pruner="kernel"); the options are checked."""
    import pytest
    import torch

    from leann_amd import gpu_graph_build as gb
    from tests.insert_ref_util import csr_equal
    from tests.util import clustered

    x = torch.from_numpy(clustered(320, 32, 3, n_centers=12, sigma=0.5))
    kw = dict(M=8, ef_construction=40, seed_nodes=256, selector="kernel", linker="kernel", search="view", inserter="kernel")
    gn, gk = gb.build_graph_gpu(x, "l2", **kw), gb.build_graph_gpu(x, "l2", assembler="kernel", **kw)
    gk.validate()
    assert csr_equal(gn, gk) and gk.cum_nneighbor_per_level.tobytes() == gn.cum_nneighbor_per_level.tobytes() and gk.max_level >= 1
    pn = gb.prune_preserving_hubs(gn, x, M=8, m_low=4, hub_fraction=0.05, pruner="kernel")
    pk = gb.prune_preserving_hubs(gn, x, M=8, m_low=4, hub_fraction=0.05, pruner="kernel", assembler="kernel")
    assert csr_equal(pn, pk) and pk.neighbors.shape[0] < gn.neighbors.shape[0]
    print(f"builder wiring: {gk.neighbors.shape[0]} links, pruned {pk.neighbors.shape[0]}: ok", flush=True)
    for bad in (dict(assembler="kernel"), dict(assembler="bogus")):  # "kernel" needs search="view"
        with pytest.raises(ValueError):
            gb.build_graph_gpu(x[:50], "l2", M=4, ef_construction=10, **bad)
    with pytest.raises(ValueError):
        gb.prune_preserving_hubs(gn, x, M=8, m_low=4, assembler="bogus")


CASES["builder_wiring"] = case_builder_wiring


if __name__ == "__main__":
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    from leann_amd import _lib

    _lib.LIB_PATH = Path(sys.argv[1])
    import torch

    torch.set_num_threads(1)
    for name in (sys.argv[2:] or list(CASES)):
        CASES[name]()
    print("ALL CASES OK")
