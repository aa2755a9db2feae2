"""lm_attn_varlen_hd32_f16 above 256 tokens on the host build of the library (tests/hip_emul/build_emul_lib.py: a thread per lane), against fp64.
The call runs in a child process: python -m tests.test_attention_long <path/to/libleann_mi355x_emul.so>"""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
LENS, HEADS = [300, 257, 40], 2


def _child(lib_path):
    import torch

    lib = C.CDLL(lib_path)
    qkv = (torch.randn((sum(LENS), 96 * HEADS), generator=torch.Generator().manual_seed(0)) * 1.5).half()

    def run(x, lens, max_len):
        cu = torch.tensor([0] + torch.tensor(lens).cumsum(0).tolist(), dtype=torch.int32)
        out = torch.zeros((x.shape[0], 32 * HEADS), dtype=torch.float16)
        assert lib.lm_attn_varlen_hd32_f16(C.c_void_p(x.data_ptr()), C.c_void_p(cu.data_ptr()), len(lens), HEADS, max_len, C.c_void_p(out.data_ptr()), None) == 0
        return out

    out, a = run(qkv, LENS, 300), 0
    for n in LENS:
        q, k, v = (qkv[a:a + n].double().view(n, 3, HEADS, 32)[:, j].transpose(0, 1) for j in range(3))
        ref = (torch.softmax(q @ k.transpose(1, 2) / 32**0.5, -1) @ v).transpose(0, 1).reshape(n, 32 * HEADS)
        err = (out[a:a + n].double() - ref).abs().max().item()
        assert err < 6e-3, (n, err)
        a += n
    assert torch.equal(out[557:], run(qkv[557:].contiguous(), [40], 40))  # the 40-token sequence: same bits from its own <= 256 launch
    print("LONG ATTENTION OK")


def test_long_attention_on_the_host_build(tmp_path_factory):
    if not Path("/opt/rocm/lib/llvm/bin/clang++").exists():
        pytest.skip("needs ROCm's clang++ as a host compiler")
    sys.path.insert(0, str(ROOT / "tests" / "hip_emul"))
    import build_emul_lib

    lib = build_emul_lib.build(tmp_path_factory.mktemp("emul_attention_long"))
    r = subprocess.run([sys.executable, "-m", "tests.test_attention_long", str(lib)], cwd=str(ROOT), capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0 and "LONG ATTENTION OK" in r.stdout, r.stdout[-3000:] + r.stderr[-5000:]


if __name__ == "__main__":
    _child(sys.argv[1])
