"""bench.py's multi-rank control flow executed BEFORE the driver's 8-GPU run does it: two ranks of the script itself, launched the way
the driver launches them (torch.distributed.run, one rank per "GPU"), over gloo, against the thread-per-lane build of the product
library (tests/hip_emul) with a tiny general-width model and corpus (`--dry-run-emulated`, a test-only switch of bench.py).  What runs:
rank-0 index build + broadcast of X and of the graph, global_batch / PartitionedSearch with its packed all_gather, the all_reduce of
elapsed / recall, the memo-off steps, `rccl_ranks` in the line -- every `world > 1` branch.  Nothing in the line is a measurement
(data = "dry-run").  SURVEY 8(e); the same for the sharded config: scripts/bench_c4.py."""
import json
import os
import socket
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
CLANG = Path("/opt/rocm/lib/llvm/bin/clang++")
sys.path.insert(0, str(ROOT / "tests" / "hip_emul"))


@pytest.fixture(scope="module")
def emul_lib(tmp_path_factory, built_libs):
    if not CLANG.exists():
        pytest.skip("needs ROCm's clang++ as a host compiler")
    import build_emul_lib

    return build_emul_lib.build(tmp_path_factory.mktemp("emul_lib_bench"))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run(cmd, timeout):
    env = {k: v for k, v in os.environ.items() if not k.startswith("LEANN_MI355X_")}
    env["PYTHONPATH"] = str(ROOT)
    return subprocess.run(cmd, cwd=str(ROOT), env=env, capture_output=True, text=True, timeout=timeout)


def _last_json(stdout):
    lines = [l for l in stdout.splitlines() if l.startswith("{")]
    assert lines, stdout[-2000:]
    return json.loads(lines[-1])


def test_bench_py_control_flow_on_two_ranks(emul_lib, world=2):
    common = ["bench.py", "--gpus", str(world), "--steps", "1", "--warmup", "1", "--chunks", "200", "--batch", "2", "--M", "8", "--efc", "24", "--ef", "16",
              "--full", "--no-cpu-baseline", "--no-table-roofline", "--no-parity-check", "--no-latency-rows", "--no-min-ef-step", "--dry-run-emulated", str(emul_lib)]
    if world == 1:
        cmd = [sys.executable] + common
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
               "--master-port", str(_free_port())] + common
    r = _run(cmd, 900)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    line = _last_json(r.stdout)
    assert line["dry_run"] is True and line["data"].startswith("dry-run")
    assert line["n_gpus"] == world and line["config"]["rccl_ranks"] == world and line["config"]["queries_per_step"] == 2 * world
    assert line["steps"] == 1 and line["value"] > 0 and line["scaling"] == "weak"
    assert 0.0 <= line["recall_at_10"] <= 1.0
    nm = line["without_call_memo"]
    assert nm["labels_identical_to_the_memo_steps"] is True and nm["value"] > 0  # all_reduce'd over the ranks
    assert line["roofline"]["bound"] in ("mfma", "hbm")
    assert r.stdout.count("\n{") + r.stdout.startswith("{") == 1  # ONE line, rank 0 only


def test_bench_py_plain_run_and_dump_outputs(emul_lib, tmp_path):
    """A plain run (no --full) times --steps steps and measures nothing else; --dump-outputs writes what the last timed step returned, and
    two runs with the same arguments write the same arrays."""
    common = [sys.executable, "bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1", "--chunks", "200", "--batch", "2", "--M", "8", "--efc", "24",
              "--ef", "16", "--dry-run-emulated", str(emul_lib), "--dump-outputs"]
    dumps = []
    for i in range(2):
        r = _run(common + [str(tmp_path / f"run{i}")], 900)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
        line = _last_json(r.stdout)
        assert line["steps"] == 2 and line["warmup"] == 1 and line["value"] > 0 and line["ms_per_step"] > 0
        assert line["unit"] == "queries/s" and line["higher_is_better"] is True and line["dtype"] == "fp16" and "recall_at_10" in line
        for k in ("without_call_memo", "roofline_distance_kernel", "roofline_encoder", "ef_sweep", "cpu_baseline", "parity_check", "small_batch_latency"):
            assert k not in line, k
        d, l = np.load(tmp_path / f"run{i}" / "distances.npy"), np.load(tmp_path / f"run{i}" / "labels.npy")
        assert d.dtype == np.float32 and l.dtype == np.float64 and d.shape == l.shape == (2, 10)
        assert np.all(l >= -1) and np.all(l < 200) and np.array_equal(l, np.rint(l))
        dumps.append((d, l))
    assert np.array_equal(dumps[0][0], dumps[1][0]) and np.array_equal(dumps[0][1], dumps[1][1])


def test_bench_host_corpus_is_the_serial_corpus():
    """bench.py generates the numpy corpus and the queries in worker processes: the same bits as SyntheticCorpus.chunks() / .queries()."""
    sys.path.insert(0, str(ROOT))
    import bench
    from leann_amd.synth import CorpusSpec, SyntheticCorpus

    c = SyntheticCorpus(CorpusSpec(n_chunks=3 * bench.CORPUS_BLOCK + 17, seed=1234, len_mean=12.0, len_std=4.0, len_min=4, len_max=24))
    h = bench._HostCorpus(c, 300)
    tok, off = h.chunks()
    qt, qo, qd = h.queries()
    tok2, off2 = c.chunks()
    qt2, qo2, qd2 = c.queries(300, seed=4321)
    for a, b in ((tok, tok2), (off, off2), (qt, qt2), (qo, qo2), (qd, qd2)):
        assert a.dtype == b.dtype and np.array_equal(a, b)


def test_bench_c4_sharded_control_flow_on_two_ranks(emul_lib):
    """scripts/bench_c4.py (BASELINE configs[3]: sharded graph, every rank searches all queries on its shard, ONE packed all_gather +
    the lm_topk_merge kernel inside the timed region) on two gloo ranks over the emulated library."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           "scripts/bench_c4.py", "--chunks", "300", "--batch", "2", "--steps", "1", "--warmup", "1", "--M", "8", "--efc", "24", "--ef", "16", "--no-cpu-baseline",
           "--no-parity-check", "--dry-run-emulated", str(emul_lib)]
    r = _run(cmd, 900)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    line = _last_json(r.stdout)
    assert line["dry_run"] is True and line["n_gpus"] == 2 and line["rccl_ranks"] == 2 and line["config"]["shard_chunks"] == 150
    assert line["value"] > 0 and line["allgather_plus_merge_us"] > 0 and line["exchange_bytes_per_rank"] == 2 * 10 * 12
    assert line["recall_at_10"] >= 0.2  # merged answer over both shards vs the exact top-10 over both shards; a random one-layer model clusters its embeddings (bit-equality of the merge itself: tests/emulated_two_rank.py)
