"""bf16 conv fwd / dgrad on the 128x128 block tile (k_conv_fwd_{db,sb}_wide,
k_conv_dgrad_{db,sb}_wide).

Small shapes that reach every way the wide kernels can go: chunk counts 1 / 2 /
odd / even, an M tail (64 rows of a 128-row tile) and M = 128 exactly, the
ragged last chunk with its per-instruction decode, a 16-channel dgrad gather,
several tiles in both directions, the stride-2 parity classes (with an M tail,
and the 1x1 kernel's classes that have no tap and must write zeros), K = 4608
and the generic-stride dgrad.

Fresh child processes run all cases, one with TNN_CONV_WIDE=2 (the wide tile
wherever it is eligible) and one with TNN_CONV_WIDE=0 (the 128x64 routes); the
switch is read once per process. The wide child's route names prove that the
wide kernels ran. Both tiles stage the same swizzled images and accumulate
every output element over the same chunks, k-steps and MFMA sequence, so y,
relu(y) and dx must be equal bit for bit; only the statistics, summed with
atomics over a different set of tiles, may differ in the last bits. Which of
the two wide forms a shape takes (double buffer or one buffer pair) is the
launcher's choice, so two more children pin it with TNN_CONV_WIDE_BUF=1 and =2:
every case then runs through both forms of every wide kernel it is eligible
for, under the same checks.

Bounds: y, relu(y) and dx against torch in fp32 on the same bf16 inputs at
3e-2 (tests/test_gpu_numerics.py TOL[bfloat16], unscaled); the fused statistics
against the fp32 sums of the kernel's own y at 2e-2, on inputs scaled by 2^-4
as tests/test_gpu_conv_db.py explains (M <= 256 rows here: the rounding of y
gives sigma ~ sqrt(256) * 2^-9 * rms(y) / sqrt(3) < 8e-3 at rms(y) <= 7/16).
test_reference_meets_its_bounds shows on the CPU that an exact kernel (the
fp32 reference rounded once to bf16) passes all of them on these inputs.
"""

import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
TOL_BF16 = 3e-2     # tests/test_gpu_numerics.py TOL[torch.bfloat16]
TOL_STATS = 2e-2    # tests/test_gpu_conv_db.py TOL_STATS
STATS_SCALE = 2.0 ** -4

# (N, H, W, Cin, Cout, K, S, P)
CASES = [
    (1, 8, 8, 64, 128, 1, 1, 0),     # 1 chunk, M tail 64 < 128
    (1, 8, 8, 128, 128, 1, 1, 0),    # 2 chunks
    (1, 8, 8, 64, 128, 3, 1, 1),     # 9 chunks (odd)
    (2, 8, 8, 128, 128, 3, 1, 1),    # M = 128 exactly, 18 chunks; both wide
    (1, 8, 8, 16, 128, 3, 1, 1),     # fwd wide; ragged last chunk
    (1, 8, 8, 128, 16, 3, 1, 1),     # dgrad wide with a 16-channel gather
    (4, 8, 8, 128, 256, 3, 1, 1),    # fwd: several tiles both ways
    (4, 8, 8, 256, 128, 3, 1, 1),    # dgrad with two n-tiles
    (4, 8, 8, 128, 256, 3, 2, 1),    # stride 2, dgrad parity classes, M tail
    (2, 8, 8, 128, 256, 1, 2, 0),    # 1x1 stride 2, the K == 0 classes
    (1, 4, 4, 512, 512, 3, 1, 1),    # K = 4608
    (1, 16, 16, 128, 128, 3, 4, 1),  # generic-stride dgrad
]
IDS = ["x".join(map(str, c)) for c in CASES]
KEYS = ("y", "y_relu", "y_stats", "dx")


def fwd_eligible(case):
    # all cases are bf16, all-pow2 with Cin % 8 == 0: the DMA-staged route
    return case[4] % 128 == 0


def dgrad_eligible(case):
    N, H, W, Ci, Co, K, S, P = case
    return Ci % 128 == 0 and K * K * Co <= 4608   # TNN_DB_MAXK_DGRAD


def relerr(a, b):
    a, b = a.float(), b.float()
    return ((a - b).abs() / (b.abs().clamp_min(1.0))).max().item()


def _inputs(idx):
    # CPU generator: both child processes must see the very same bits
    N, H, W, Ci, Co, K, S, P = CASES[idx]
    g = torch.Generator().manual_seed(300 + idx)
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
        xs, bs = x * STATS_SCALE, bias * STATS_SCALE
        y_stats, stats = ext.conv2d_fwd_stats(xs, w, bs, S, S, P, P)
        out.append({
            "fwd_route": ext.conv2d_fwd_route(x, w, S, S, P, P, False),
            "fwd_stats_route": ext.conv2d_fwd_route(xs, w, S, S, P, P, True),
            "dgrad_route": ext.conv2d_dgrad_route(dy, w, H, W, S, S, P, P),
            "y": ext.conv2d_fwd(x, w, bias, S, S, P, P, False).cpu(),
            "y_relu": ext.conv2d_fwd(x, w, bias, S, S, P, P, True).cpu(),
            "y_stats": y_stats.cpu(),
            "y_scaled": ext.conv2d_fwd(xs, w, bs, S, S, P, P, False).cpu(),
            "stats": stats.cpu(),
            "dx": ext.conv2d_dgrad(dy, w, H, W, S, S, P, P).cpu(),
        })
    torch.cuda.synchronize()
    return out


def _child(tmp_path_factory, mode, buf="0"):
    path = str(tmp_path_factory.mktemp("conv_wide") / f"wide{mode}{buf}.pt")
    env = dict(os.environ, TNN_CONV_WIDE=mode, TNN_CONV_WIDE_BUF=buf)
    for name in ("TNN_FWD_DB", "TNN_DB_MAXK", "TNN_DB_MAXK_DGRAD"):
        env.pop(name, None)
    subprocess.run([sys.executable, os.path.abspath(__file__), path],
                   env=env, check=True, timeout=300)
    return torch.load(path)


@pytest.fixture(scope="module")
def wide_out(tmp_path_factory):
    return _child(tmp_path_factory, "2")


@pytest.fixture(scope="module")
def narrow_out(tmp_path_factory):
    return _child(tmp_path_factory, "0")


# the wide children: the launcher's own choice of buffering, then each form
WIDE = {"auto": "0", "db": "1", "sb": "2"}


@pytest.fixture(scope="module", params=list(WIDE))
def wide_any(request, tmp_path_factory, wide_out):
    if request.param == "auto":
        return request.param, wide_out
    return request.param, _child(tmp_path_factory, "2", WIDE[request.param])


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


def _check(case, got, ref):
    """Every bound of this module, for one case's outputs."""
    Co = case[4]
    errs = {
        "y": relerr(got["y"], ref["y"]),
        "y_relu": relerr(got["y_relu"], ref["y"].clamp_min(0)),
        "y_stats": relerr(got["y_stats"], ref["y"] * STATS_SCALE),
        "dx": relerr(got["dx"], ref["dx"]),
    }
    print(case, errs)
    for key, err in errs.items():
        assert err < TOL_BF16, (case, key, errs)
    # fused statistics against the fp32 sums of the returned y
    stats = got["stats"]
    assert stats.numel() == 2 * Co, "fused-statistics route expected"
    yf = got["y_stats"].float().reshape(-1, Co)
    e0, e1 = relerr(stats[0], yf.sum(0)), relerr(stats[1], (yf * yf).sum(0))
    print(case, "stats", e0, e1)
    assert e0 < TOL_STATS and e1 < TOL_STATS, (case, e0, e1)


@pytest.mark.parametrize("idx", range(len(CASES)), ids=IDS)
def test_reference_meets_its_bounds(idx, torch_ref):
    """No GPU: an exact kernel -- fp32 results rounded once to bf16, the
    statistics summed in fp32 before that rounding -- passes every bound."""
    ref = torch_ref[idx]
    Co = CASES[idx][4]
    ys = ref["y"] * STATS_SCALE
    ysf = ys.reshape(-1, Co)
    _check(CASES[idx], {
        "y": ref["y"].bfloat16(),
        "y_relu": ref["y"].clamp_min(0).bfloat16(),
        "y_stats": ys.bfloat16(),
        "stats": torch.stack([ysf.sum(0), (ysf * ysf).sum(0)]),
        "dx": ref["dx"].bfloat16(),
    }, ref)


ROUTES = ("fwd_route", "fwd_stats_route", "dgrad_route")


@pytest.mark.gpu
@pytest.mark.parametrize("idx", range(len(CASES)), ids=IDS)
def test_conv_wide_routes(idx, wide_any, narrow_out):
    case = CASES[idx]
    assert fwd_eligible(case) or dgrad_eligible(case), case
    form, out = wide_any
    wide, narrow = out[idx], narrow_out[idx]
    print(case, form, [wide[r] for r in ROUTES], "|",
          [narrow[r] for r in ROUTES])
    for r in ROUTES:
        eligible = dgrad_eligible(case) if r == "dgrad_route" \
            else fwd_eligible(case)
        assert ("wide" in wide[r]) == eligible, (case, r, wide[r])
        if eligible and form != "auto":
            assert f"_{form}_wide" in wide[r], (case, r, wide[r])
        assert "wide" not in narrow[r], (case, r, narrow[r])


@pytest.mark.gpu
@pytest.mark.parametrize("idx", range(len(CASES)), ids=IDS)
def test_conv_wide_vs_torch(idx, wide_any, torch_ref):
    got = wide_any[1][idx]
    _check(CASES[idx], got, torch_ref[idx])
    # the y returned with the statistics is the plain y of the same inputs
    assert torch.equal(got["y_stats"], got["y_scaled"]), CASES[idx]


@pytest.mark.gpu
@pytest.mark.parametrize("idx", range(len(CASES)), ids=IDS)
def test_conv_wide_bitwise_vs_narrow(idx, wide_any, narrow_out):
    got, ref = wide_any[1][idx], narrow_out[idx]
    for key in KEYS:
        assert torch.equal(got[key], ref[key]), (CASES[idx], key, relerr(
            got[key], ref[key]))


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    torch.save(_run_all(), sys.argv[1])
