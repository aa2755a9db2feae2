"""lm_graph_add_links -- the link insertion of graph construction as HIP kernels -- on the CPU: the product library built for the host
(tests/hip_emul/build_emul_lib.py, a thread per lane) against tests/link_ref/lm_link_ref.c, an independent C restatement whose shrink
step is tests/select_ref/lm_select_ref.c and whose distance function is the oracle's orc_dist.  The scenarios live in
tests/emulated_link_cases.py and run in a child process that loads the emulated library: kernel against restatement (adj, dist bits and
deg byte for byte; repeated and reordered calls), three-way agreement with the builder's torch form, the builder's `linker` wiring,
argument checking."""
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CLANG = Path("/opt/rocm/lib/llvm/bin/clang++")
sys.path.insert(0, str(ROOT / "tests" / "hip_emul"))


@pytest.fixture(scope="module")
def libs(tmp_path_factory, built_libs):
    if not CLANG.exists():
        pytest.skip("needs ROCm's clang++ as a host compiler")
    import build_emul_lib

    from tests.link_ref_util import compile_ref

    d = tmp_path_factory.mktemp("emul_link")
    return build_emul_lib.build(d), compile_ref(d)


def _run(libs, *cases, timeout=1800):
    r = subprocess.run([sys.executable, "-m", "tests.emulated_link_cases", str(libs[0]), str(libs[1]), *cases], cwd=str(ROOT), capture_output=True,
                       text=True, timeout=timeout)
    assert r.returncode == 0 and "ALL CASES OK" in r.stdout, r.stdout[-3000:] + r.stderr[-5000:]
    assert "MISMATCH" not in r.stdout
    return r.stdout


def test_kernel_matches_the_c_restatement(libs):
    out = _run(libs, "kernel_vs_restatement")
    assert out.count(": ok") >= 80


def test_torch_form_restatement_and_kernel_agree(libs):
    out = _run(libs, "torch_form_agrees")
    assert out.count(": ok") >= 24


def test_builder_and_pruning_give_the_same_graph_with_either_linker(libs):
    _run(libs, "builder_wiring")


def test_rejected_arguments_and_unknown_linker(libs):
    _run(libs, "argument_checking")


def test_default_linker_is_the_torch_path(monkeypatch):
    """The default does not change: build_graph_gpu / prune_preserving_hubs / _LevelGraph default to linker="torch" (and a level graph
    then keeps the int64 / similarity layout it always had), the backend's gpu_link_kernel to False."""
    import inspect

    import torch

    from leann_amd import backend
    from leann_amd import gpu_graph_build as gb

    for f in (gb.build_graph_gpu, gb.prune_preserving_hubs, gb._LevelGraph.__init__):
        assert inspect.signature(f).parameters["linker"].default == "torch"
    G = gb._LevelGraph(torch.arange(5), 3)
    assert G.linker == "torch" and G.adj.dtype == torch.int64 and G.sim.dtype == torch.float32 and not hasattr(G, "dist")
    # the backend without the build parameter: the pruning step (the host builder's graph, CPU tensors) is handed linker="torch"
    import numpy as np

    seen = {}
    real = gb.prune_preserving_hubs

    def recording(g, x, M, m_low, hub_fraction=0.02, **kw):
        seen.update(kw)
        return real(g, x, M, m_low, hub_fraction, **kw)

    monkeypatch.setattr(gb, "prune_preserving_hubs", recording)
    b = backend.Mi355xBuilder(M=4, efConstruction=10, hub_preserving_m=2, gpu_build_threshold=10**9)
    g = b._build_graph(np.random.default_rng(0).standard_normal((60, 8)).astype(np.float32), "mips")
    g.validate()
    assert seen == {"selector": "torch", "linker": "torch"}
