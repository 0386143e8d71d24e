"""conv2d_wgrad_bias: weight and bias gradient from one wgrad launch.

The bias gradient db[co] = sum_m dy[m][co] is written by the wgrad kernel as
one more row of its split-K slab, so dw and db come out of one kernel and one
reduce. Checked against torch.nn.grad.conv2d_weight in float64 on the CPU,
from the bf16-rounded inputs, over every output element.

Tolerance (derived, not measured): products of two bf16 values are exact in
fp32, and an fp32 sum of M terms in any order is within
(M-1) * 2^-24 * sum|terms| of the exact sum. With S the same reference run
on absolute values, |dw - ref| <= 2 * M * 2^-24 * S + 1e-30 element-wise
(the factor 2 covers the MFMA's internal accumulation order), and likewise
|db - sum dy| <= 2 * M * 2^-24 * sum|dy|. A bf16 output adds one bf16 ulp,
bounded by 2^-7 * |ref|.
"""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from tnn_amd import _C, ops
    ext = _C.ext()

DEV = "cuda"
EPS = 2.0 ** -24
BF16_ULP = 2.0 ** -7

# (N, H, W, Cin, Cout, K, stride, pad)
CASES = {
    # M=16 < BK, Kout=72 < BM, Cout=8 < BN: every tail at once
    "tails": (1, 4, 4, 8, 8, 3, 1, 1),
    # 9 tile-rows, one split, exact tiles
    "exact": (2, 8, 8, 128, 64, 3, 1, 1),
    # Kout=144 (ragged second tile-row), two n-tiles, 4 splits
    "ragged": (4, 16, 16, 16, 128, 3, 1, 1),
    # M=8192, 72 base tiles -> 29 splits starting at multiples of 282.48
    "splits29": (32, 16, 16, 256, 256, 3, 1, 1),
    "stride2": (4, 16, 16, 128, 256, 3, 2, 1),
    "shortcut": (4, 16, 16, 128, 256, 1, 2, 0),
    # not pow2: the non-vector fallback kernel
    "nonpow2": (2, 9, 9, 24, 40, 3, 2, 1),
}
IDS = list(CASES)


def _ref(x, dy, K, S, P):
    """float64 CPU reference and its absolute-value twin, NHWC-shaped."""
    Ci, Co = x.shape[-1], dy.shape[-1]
    xd = x.detach().cpu().double().permute(0, 3, 1, 2)
    dyd = dy.detach().cpu().double().permute(0, 3, 1, 2)

    def wg(a, b):
        r = torch.nn.grad.conv2d_weight(a, (Co, Ci, K, K), b, stride=S,
                                        padding=P)
        return r.permute(2, 3, 1, 0)  # -> [KH,KW,Ci,Co]

    M = dy.numel() // Co
    return {
        "M": M,
        "dw": wg(xd, dyd), "dw_abs": wg(xd.abs(), dyd.abs()),
        "db": dyd.sum(dim=(0, 2, 3)), "db_abs": dyd.abs().sum(dim=(0, 2, 3)),
    }


@functools.lru_cache(maxsize=None)
def _case(name, dtype=torch.bfloat16):
    """Inputs, one float64 reference and the kernel's fp32 result per case,
    computed once and shared (read-only) by the tests below. fp32 inputs
    hold the same bf16-rounded values, so their products stay exact in fp32
    and the bound above holds as written."""
    N, H, W, Ci, Co, K, S, P = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    OH = (H + 2 * P - K) // S + 1
    OW = (W + 2 * P - K) // S + 1
    x = torch.randn(N, H, W, Ci, generator=g).bfloat16().to(dtype).to(DEV)
    dy = torch.randn(N, OH, OW, Co, generator=g).bfloat16().to(dtype).to(DEV)
    ref = _ref(x, dy, K, S, P)
    dw, db = ext.conv2d_wgrad_bias(x, dy, K, K, S, S, P, P, False)
    return x, dy, ref, dw, db


def _check(dw, db, ref, extra_rel=0.0):
    M = ref["M"]
    err = (dw.detach().cpu().double() - ref["dw"]).abs()
    bound = 2 * M * EPS * ref["dw_abs"] + extra_rel * ref["dw"].abs() + 1e-30
    worst = (err / bound).max().item()
    print(f"dw: max err/bound {worst:.3g}, max err {err.max().item():.3g}")
    assert (err <= bound).all(), f"dw off: err/bound {worst}"
    err = (db.detach().cpu().double() - ref["db"]).abs()
    bound = 2 * M * EPS * ref["db_abs"] + extra_rel * ref["db"].abs() + 1e-30
    worst = (err / bound).max().item()
    print(f"db: max err/bound {worst:.3g}, max err {err.max().item():.3g}")
    assert (err <= bound).all(), f"db off: err/bound {worst}"


@pytest.mark.parametrize("name", IDS)
def test_wgrad_bias_fp32_out(name):
    x, dy, ref, dw, db = _case(name)
    N, H, W, Ci, Co, K, S, P = CASES[name]
    assert dw.shape == (K, K, Ci, Co) and dw.dtype == torch.float32
    assert db.shape == (Co,) and db.dtype == torch.float32
    _check(dw, db, ref)


@pytest.mark.parametrize("name", ["tails", "exact", "stride2", "nonpow2"])
def test_wgrad_bias_fp32_out_fp32_in(name):
    """the bias row of the fp32 kernels (vector route and generic fallback)"""
    x, dy, ref, dw, db = _case(name, torch.float32)
    N, H, W, Ci, Co, K, S, P = CASES[name]
    assert x.dtype == torch.float32 and dy.dtype == torch.float32
    assert dw.shape == (K, K, Ci, Co) and dw.dtype == torch.float32
    assert db.shape == (Co,) and db.dtype == torch.float32
    _check(dw, db, ref)


@pytest.mark.parametrize("name", IDS)
def test_wgrad_bias_bf16_out(name):
    x, dy, ref, dw32, db32 = _case(name)
    K, S, P = CASES[name][5:]
    dw, db = ext.conv2d_wgrad_bias(x, dy, K, K, S, S, P, P, True)
    assert dw.dtype == torch.bfloat16 and db.dtype == torch.bfloat16
    for got, f32 in ((dw, dw32), (db, db32)):
        d = (got.float() - f32.bfloat16().float()).abs()
        assert (d <= BF16_ULP * f32.abs() + 1e-30).all(), d.max().item()


@pytest.mark.parametrize("name", ["exact", "ragged", "splits29"])
def test_wgrad_alone_bit_identical(name):
    x, dy, ref, dw, db = _case(name)
    K, S, P = CASES[name][5:]
    alone = ext.conv2d_wgrad(x, dy, K, K, S, S, P, P, False)
    assert torch.equal(alone, dw)
    alone_bf = ext.conv2d_wgrad(x, dy, K, K, S, S, P, P, True)
    dw_bf, _ = ext.conv2d_wgrad_bias(x, dy, K, K, S, S, P, P, True)
    assert torch.equal(alone_bf, dw_bf)


@pytest.mark.parametrize("name", IDS)
def test_wgrad_bias_repeatable(name):
    x, dy, ref, dw, db = _case(name)
    K, S, P = CASES[name][5:]
    dw2, db2 = ext.conv2d_wgrad_bias(x, dy, K, K, S, S, P, P, False)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)
    a = ext.conv2d_wgrad(x, dy, K, K, S, S, P, P, False)
    b = ext.conv2d_wgrad(x, dy, K, K, S, S, P, P, False)
    assert torch.equal(a, b)


@pytest.mark.parametrize("cin", [16, 3], ids=["cin16", "stem_cin3"])
@pytest.mark.parametrize("fuse_relu", [False, True], ids=["linear", "relu"])
def test_autograd_conv_bias(fuse_relu, cin):
    N, H, W, Co, K, S, P = 4, 16, 16, 128, 3, 1, 1
    g = torch.Generator().manual_seed(11 + cin)
    x = torch.randn(N, H, W, cin, generator=g).bfloat16().to(DEV)
    w = (torch.randn(K, K, cin, Co, generator=g) * 0.1).bfloat16().to(DEV)
    b = torch.randn(Co, generator=g).bfloat16().to(DEV)
    up = torch.randn(N, H, W, Co, generator=g).bfloat16().to(DEV)
    w.requires_grad_(True)
    b.requires_grad_(True)
    y = ops.conv2d_nhwc(x, w, b, (S, S), (P, P), fuse_relu=fuse_relu)
    y.backward(up)
    assert w.grad.shape == w.shape and b.grad.shape == b.shape
    # the ReLU mask applies to dy before both gradients
    dy = up * (y.detach() > 0) if fuse_relu else up
    ref = _ref(x, dy, K, S, P)
    _check(w.grad, b.grad, ref, extra_rel=BF16_ULP)


def test_autograd_bias_only_keeps_colsum():
    """weight frozen: no wgrad runs, the bias gradient is the plain colsum"""
    N, H, W, Ci, Co, K = 2, 8, 8, 16, 32, 3
    g = torch.Generator().manual_seed(3)
    x = torch.randn(N, H, W, Ci, generator=g).bfloat16().to(DEV)
    w = (torch.randn(K, K, Ci, Co, generator=g) * 0.1).bfloat16().to(DEV)
    b = torch.randn(Co, generator=g).bfloat16().to(DEV).requires_grad_(True)
    up = torch.randn(N, H, W, Co, generator=g).bfloat16().to(DEV)
    ops.conv2d_nhwc(x, w, b, (1, 1), (1, 1)).backward(up)
    ref = up.cpu().double().sum(dim=(0, 1, 2))
    ref_abs = up.cpu().double().abs().sum(dim=(0, 1, 2))
    err = (b.grad.cpu().double() - ref).abs()
    M = N * H * W
    assert (err <= 2 * M * EPS * ref_abs + BF16_ULP * ref.abs() + 1e-30).all()
