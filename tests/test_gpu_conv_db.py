"""bf16 double-buffered conv fwd / dgrad k-loop (k_conv_fwd_db, k_conv_dgrad_db).

Small shapes that reach every way the loop can go: chunk counts 1 / 2 / odd /
even, chunks that span several (kh,kw) slices, the ragged last chunk, M and
Cout tails, several tiles, stride 2 (dgrad parity route), 1x1 stride 2, the
K = 4608 deep-layer shape, and stride 4 (the dgrad kernels that test the
stride divisibility at run time).

Every case is checked twice: against torch in fp32 on the same bf16 inputs,
and bitwise against the same build routed to the single-buffer kernels with
TNN_FWD_DB=0. Both routes accumulate the same chunks in the same order
through the same MFMA sequence and share the epilogue, so the outputs must be
equal bit for bit. The switch is read once per process, so the second route
runs in one fresh child process that covers all cases.
"""

import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
TOL_BF16 = 3e-2     # tests/test_gpu_numerics.py TOL[torch.bfloat16]
TOL_STATS = 2e-2    # tests/test_gpu_numerics.py test_conv_fwd_fused_bn_stats
# The statistics are summed from the fp32 accumulators, the reference from
# the bf16-rounded y, and relerr() is absolute (2e-2) for |sum| < 1. At these
# row counts (M <= 128) the rounding of y alone would reach that: per element
# up to 2^-9 |y|, i.e. sigma ~ sqrt(128) * 2^-9 * rms(y) / sqrt(3) = 0.013 *
# rms(y), with rms(y) up to 7 here. The statistics call therefore runs on
# x and bias scaled by 2^-4 (exact in bf16 and in the fp32 accumulation, so
# its y must equal the unscaled y times 2^-4 bit for bit), which puts the
# rounding noise at sigma < 6e-3, a third of the bound.
STATS_SCALE = 2.0 ** -4

# (N, H, W, Cin, Cout, K, S, P)
CASES = [
    (1, 8, 8, 64, 64, 1, 1, 0),      # chunk count 1
    (1, 8, 8, 128, 64, 1, 1, 0),     # chunk count 2
    (1, 8, 8, 64, 64, 3, 1, 1),      # chunk count 9 (odd)
    (1, 8, 8, 128, 64, 3, 1, 1),     # chunk count 18 (even)
    (1, 8, 8, 16, 64, 3, 1, 1),      # K = 144: ragged last chunk, mixed slices
    (1, 8, 8, 32, 64, 3, 1, 1),      # chunks span several (kh,kw) slices
    (1, 4, 4, 64, 16, 3, 1, 1),      # M tail (16 < 128), Cout tail (16 < 64)
    (2, 8, 8, 64, 128, 3, 1, 1),     # several tiles in both directions
    (2, 8, 8, 64, 128, 3, 2, 1),     # fwd stride 2; dgrad parity route
    (2, 8, 8, 64, 128, 1, 2, 0),     # 1x1 stride 2
    (1, 4, 4, 512, 512, 3, 1, 1),    # K = 4608
    (1, 16, 16, 64, 64, 3, 4, 1),    # stride 4: dgrad generic-stride route
]
IDS = ["x".join(map(str, c)) for c in CASES]


def relerr(a, b):
    a, b = a.float(), b.float()
    return ((a - b).abs() / (b.abs().clamp_min(1.0))).max().item()


def _inputs(idx):
    # CPU generator: the child process must see the very same bits
    N, H, W, Ci, Co, K, S, P = CASES[idx]
    g = torch.Generator().manual_seed(100 + idx)
    OH = (H + 2 * P - K) // S + 1
    x = torch.randn(N, H, W, Ci, generator=g).bfloat16()
    w = (torch.randn(K, K, Ci, Co, generator=g) * 0.1).bfloat16()
    bias = torch.randn(Co, generator=g).bfloat16()
    dy = torch.randn(N, OH, OH, Co, generator=g).bfloat16()
    return x, w, bias, dy


def _run_all():
    from tnn_amd import _C
    ext = _C.ext()
    out = []
    for idx, (N, H, W, Ci, Co, K, S, P) in enumerate(CASES):
        x, w, bias, dy = (t.to(DEV) for t in _inputs(idx))
        y, stats = ext.conv2d_fwd_stats(x * STATS_SCALE, w, bias * STATS_SCALE,
                                        S, S, P, P)
        out.append({
            "y": ext.conv2d_fwd(x, w, bias, S, S, P, P, False).cpu(),
            "y_relu": ext.conv2d_fwd(x, w, bias, S, S, P, P, True).cpu(),
            "y_stats": y.cpu(),
            "stats": stats.cpu(),
            "dx": ext.conv2d_dgrad(dy, w, H, W, S, S, P, P).cpu(),
        })
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def db_out():
    assert os.environ.get("TNN_FWD_DB", "1") != "0", \
        "this module compares the default route against TNN_FWD_DB=0"
    return _run_all()


@pytest.fixture(scope="module")
def single_out(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("conv_db") / "single.pt")
    env = dict(os.environ, TNN_FWD_DB="0")
    subprocess.run([sys.executable, os.path.abspath(__file__), path],
                   env=env, check=True, timeout=300)
    return torch.load(path)


@pytest.fixture(scope="module")
def torch_ref():
    F = torch.nn.functional
    out = []
    for idx, (N, H, W, Ci, Co, K, S, P) in enumerate(CASES):
        x, w, bias, dy = _inputs(idx)
        wf = w.permute(3, 2, 0, 1).float()
        y = F.conv2d(x.permute(0, 3, 1, 2).float(), wf, bias.float(),
                     stride=S, padding=P).permute(0, 2, 3, 1)
        dx = torch.nn.grad.conv2d_input(
            (N, Ci, H, W), wf, dy.permute(0, 3, 1, 2).float(), stride=S,
            padding=P).permute(0, 2, 3, 1)
        out.append({"y": y, "dx": dx})
    return out


@pytest.mark.parametrize("idx", range(len(CASES)), ids=IDS)
def test_conv_db_vs_torch(idx, db_out, torch_ref):
    N, H, W, Ci, Co, K, S, P = CASES[idx]
    got, ref = db_out[idx], torch_ref[idx]
    tol_f = TOL_BF16 * max(1, (K * K * Ci) // 256)
    tol_d = TOL_BF16 * max(1, (K * K * Co) // 256)
    errs = {
        "y": relerr(got["y"], ref["y"]),
        "y_relu": relerr(got["y_relu"], ref["y"].clamp_min(0)),
        "y_stats": relerr(got["y_stats"], ref["y"] * STATS_SCALE),
        "dx": relerr(got["dx"], ref["dx"]),
    }
    print(CASES[idx], errs)
    assert errs["y"] < tol_f and errs["y_relu"] < tol_f, (CASES[idx], errs)
    assert errs["y_stats"] < tol_f, (CASES[idx], errs)
    assert torch.equal(got["y_stats"], got["y"] * STATS_SCALE), CASES[idx]
    assert errs["dx"] < tol_d, (CASES[idx], errs)
    # fused statistics against the kernel's own y
    stats = got["stats"]
    assert stats.numel() == 2 * Co, "fused-statistics route expected"
    yf = got["y_stats"].float().reshape(-1, Co)
    e0, e1 = relerr(stats[0], yf.sum(0)), relerr(stats[1], (yf * yf).sum(0))
    print(CASES[idx], "stats", e0, e1)
    assert e0 < TOL_STATS and e1 < TOL_STATS, (CASES[idx], e0, e1)


@pytest.mark.parametrize("idx", range(len(CASES)), ids=IDS)
def test_conv_db_bitwise_vs_single_buffer(idx, db_out, single_out):
    got, ref = db_out[idx], single_out[idx]
    assert ref["stats"].numel() == 0, "child did not run with TNN_FWD_DB=0"
    for key in ("y", "y_relu", "y_stats", "dx"):
        assert torch.equal(got[key], ref[key]), (CASES[idx], key, relerr(
            got[key], ref[key]))


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    torch.save(_run_all(), sys.argv[1])
