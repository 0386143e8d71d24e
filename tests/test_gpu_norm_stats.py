"""Normalization statistics vs float64, at inputs whose mean dwarfs their
spread, plus the launcher branches no other test reaches.

Every norm kernel accumulates its statistics in fp32. A one-pass variance
(E[x^2] - mean^2) loses (mean/std)^2 * 2^-24 of the result to cancellation,
so at mean/std = 64 its invstd is already off by 1e-3 or more while a
two-pass or shifted form stays near 1e-6. Nothing else in the suite feeds a
norm a mean/std above 0.25, or looks at invstd at all.

All references are float64 torch on the CPU, computed from the kernel's
actual (dtype-rounded) input. Statistics are compared with

    stat_err_invstd = max |is_k - is_64| / is_64
    stat_err_mean   = max |m_k  - m_64| / std_64

and never with the clamp_min(1.0) relerr, which degenerates into an
absolute check for small values.

Bounds (set before looking at any kernel's result):

  INVSTD_BOUND = 1e-4. With strictly sequential fp32 sums (pessimistic for
    a tree-reducing kernel) two-pass measured <= 1.7e-6 and shifted one-pass
    <= 1.6e-5 over these cases; the raw one-pass form measured >= 3e-4 at
    mean/std = 64 even with pairwise sums. The bound sits 6x above the worst
    stable result and 3x below the best unstable one.
  MEAN_BOUND = 2e-3. An fp32 sum of n values near `offset` is off by about
    ulp(offset * n); sequential two-pass measured 9.3e-4 at worst.

Each case also runs the fp32 two-pass algorithm with torch on the CPU and
asserts the same bounds for it, which proves the inputs allow them.

fp32 y: the two statistic bounds pushed through xhat * gamma + beta with
|xhat| <= 8:  |y_k - y_64| <= |gamma|_max * (MEAN_BOUND + 8 * INVSTD_BOUND)
+ 1e-5. bf16 y, and everything in the offset-0 dispatch cases, uses the
suite's TOL-scaled relerr (test_gpu_numerics.test_layernorm's factors).
"""

import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from tnn_amd import _C
    ext = _C.ext()

DEV = "cuda"
EPS = 1e-5
F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]
TOL = {F32: 2e-4, BF16: 3e-2}  # same scale as test_gpu_numerics

INVSTD_BOUND = 1e-4
MEAN_BOUND = 2e-3

# (offset, std): the ratio-0 control plus mean/std of 64, 256 and 256
OFFSETS = [(0.0, 1.0), (64.0, 1.0), (256.0, 1.0), (64.0, 0.25)]


def stat_err_invstd(is_k, is_64):
    is_k = is_k.detach().double().cpu().reshape(-1)
    return ((is_k - is_64).abs() / is_64).max().item()


def stat_err_mean(m_k, m_64, std_64):
    m_k = m_k.detach().double().cpu().reshape(-1)
    return ((m_k - m_64).abs() / std_64).max().item()


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs() / b.abs().clamp_min(1.0)).max().item()


def maxabs(a, b):
    return (a.detach().double().cpu() - b.detach().double().cpu()).abs().max().item()


def ref_stats(xg):
    """float64 mean / std / invstd of each row of xg [groups, n]."""
    m = xg.mean(1)
    var = ((xg - m[:, None]) ** 2).mean(1)
    return m, var.sqrt(), (var + EPS).rsqrt()


def fp32_two_pass(xg):
    """The stable fp32 algorithm on the CPU (xg holds fp32/bf16 values, so
    .float() is exact)."""
    xf = xg.float().contiguous()
    m = xf.mean(1)
    var = ((xf - m[:, None]) ** 2).mean(1)
    return m, (var + EPS).rsqrt()


def assert_stats(tag, mean_k, invstd_k, xg):
    """mean_k / invstd_k against float64 on xg [groups, n]; returns the
    float64 (mean, invstd)."""
    m64, std64, is64 = ref_stats(xg)
    m32, is32 = fp32_two_pass(xg)
    ref_is, ref_m = stat_err_invstd(is32, is64), stat_err_mean(m32, m64, std64)
    k_is, k_m = stat_err_invstd(invstd_k, is64), stat_err_mean(mean_k, m64, std64)
    print(f"{tag}: stat_err_invstd kernel {k_is:.3e} cpu-fp32-two-pass "
          f"{ref_is:.3e} | stat_err_mean kernel {k_m:.3e} cpu-fp32-two-pass "
          f"{ref_m:.3e}")
    assert ref_is <= INVSTD_BOUND and ref_m <= MEAN_BOUND, \
        f"{tag}: inputs do not allow the bound (two-pass {ref_is:.3e}, {ref_m:.3e})"
    assert k_is <= INVSTD_BOUND, f"{tag}: stat_err_invstd {k_is:.3e}"
    assert k_m <= MEAN_BOUND, f"{tag}: stat_err_mean {k_m:.3e}"
    return m64, is64


def assert_y_offset(tag, y_k, y64, gamma64, dtype):
    if dtype == F32:
        bound = gamma64.abs().max().item() * (MEAN_BOUND + 8 * INVSTD_BOUND) + 1e-5
        err = maxabs(y_k, y64)
        print(f"{tag}: y maxabs {err:.3e} bound {bound:.3e}")
        assert err <= bound, f"{tag}: y maxabs {err:.3e} > {bound:.3e}"
    else:
        err = relerr(y_k, y64)
        print(f"{tag}: y relerr {err:.3e}")
        assert err < TOL[dtype] * 2, f"{tag}: y relerr {err:.3e}"


def _gen(seed):
    return torch.Generator().manual_seed(seed)


@functools.lru_cache(maxsize=None)
def affine(C):
    """fp32 gamma / beta shared by every case of width C (CPU)."""
    g = _gen(1000 + C)
    return torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)


@functools.lru_cache(maxsize=None)
def offset_rows(rows, D, offset, std, dtype):
    """x [rows, D] = randn * std + offset, rounded to dtype (CPU)."""
    return (torch.randn(rows, D, generator=_gen(12)) * std + offset).to(dtype)


@functools.lru_cache(maxsize=None)
def offset_nhwc(shape, offset, std, dtype, seed=13):
    """NHWC x with a different, sign-alternating offset per channel, so no
    per-tensor shift can centre it: offset * (1 + c / C) * (-1)^c."""
    C = shape[-1]
    c = torch.arange(C, dtype=torch.float32)
    off = offset * (1 + c / C) * (1 - 2 * (c % 2))
    return (torch.randn(*shape, generator=_gen(seed)) * std + off).to(dtype)


# ---------------------------------------------------------------------------
# offset inputs
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("offset,std", OFFSETS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("D", [768, 1280, 4096, 770])
def test_ln_fwd_offset(D, dtype, offset, std):
    """768: vector PK=1; 1280: PK=2 (fp32); 4096: PK=4 (fp32); 770: scalar."""
    x = offset_rows(64, D, offset, std, dtype)
    gamma, beta = affine(D)
    y, mean, invstd = ext.ln_fwd(x.to(DEV), gamma.to(DEV), beta.to(DEV), EPS)
    tag = f"ln_fwd D={D} {dtype} ({offset},{std})"
    x64 = x.double()
    m64, is64 = assert_stats(tag, mean, invstd, x64)
    y64 = (x64 - m64[:, None]) * is64[:, None] * gamma.double() + beta.double()
    assert_y_offset(tag, y, y64, gamma.double(), dtype)


@pytest.mark.parametrize("offset,std", OFFSETS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape,G", [((2, 16, 16, 64), 4), ((3, 5, 7, 48), 6)],
                         ids=["2x16x16x64-G4", "3x5x7x48-G6"])
def test_gn_fwd_offset(shape, G, dtype, offset, std):
    N, C = shape[0], shape[-1]
    x = (torch.randn(*shape, generator=_gen(14)) * std + offset).to(dtype)
    gamma, beta = affine(C)
    y, mean, invstd = ext.gn_fwd(x.to(DEV), gamma.to(DEV), beta.to(DEV), G, EPS)
    tag = f"gn_fwd {shape} G={G} {dtype} ({offset},{std})"
    x5 = x.double().reshape(N, -1, G, C // G)  # [N, HW, G, CG]
    xg = x5.permute(0, 2, 1, 3).reshape(N * G, -1)
    m64, is64 = assert_stats(tag, mean, invstd, xg)
    m5, is5 = m64.reshape(N, 1, G, 1), is64.reshape(N, 1, G, 1)
    y64 = ((x5 - m5) * is5).reshape(shape) * gamma.double() + beta.double()
    assert_y_offset(tag, y, y64, gamma.double(), dtype)


@pytest.mark.parametrize("offset,std", OFFSETS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", [64, 30, 264])
def test_bn_fwd_train_offset(C, dtype, offset, std):
    """64: vector stats; 30: scalar stats (both dtypes); 264: a channel
    block wider than the 256 threads that fold it."""
    shape = (8, 16, 16, C)
    x = offset_nhwc(shape, offset, std, dtype)
    gamma, beta = affine(C)
    y, mean, invstd = ext.bn_fwd_train(x.to(DEV), gamma.to(DEV), beta.to(DEV),
                                       None, None, 0.1, EPS, False, 0.0, 0,
                                       None)
    tag = f"bn_fwd_train C={C} {dtype} ({offset},{std})"
    x64 = x.double().reshape(-1, C)
    m64, is64 = assert_stats(tag, mean, invstd, x64.t())
    y64 = ((x64 - m64) * is64 * gamma.double() + beta.double()).reshape(shape)
    assert_y_offset(tag, y, y64, gamma.double(), dtype)


def check_fused_ln_gemm(M, K, dtype, offset, std):
    """LayerNorm prologue of the decode GEMMs: M=1 ext.gemm (LDS matvec),
    M=2 ext.gemm_skinny VALU form, M=8 its bf16 MFMA form (VALU for fp32).

    Tolerance: the unfused pipeline with float64 statistics, rounded the way
    the dtype forces (layer_norm in float64 -> round -> GEMM in float64 ->
    round), has some maximum error against the unrounded float64 result.
    The kernel gets 4x that + 1e-6; the 4x covers fp32 accumulation order
    over K = 768 and is a margin over the reference, not a measurement.

    In bf16 that pipeline error (1e-2) is the rounding of the normalised row
    and of the output, coarser than what a 1% error in invstd does, so the
    bf16 cases hold the kernels to the pipeline but cannot tell a one-pass
    variance from a stable one. The fp32 cases can, and they also need the
    mean to better than its own fp32 rounding (half an ulp of 256 is 1.5e-5
    of a std, summed coherently over K by the GEMM).
    """
    N = 256
    x = offset_rows(M, K, offset, std, dtype)
    g = _gen(15)
    w = (torch.randn(K, N, generator=g) / K ** 0.5).to(dtype)
    bias = torch.randn(N, generator=g).to(dtype)
    gamma, beta = affine(K)
    ln64 = F.layer_norm(x.double(), (K,), gamma.double(), beta.double(), EPS)
    ref = ln64 @ w.double() + bias.double()
    pipe = (ln64.to(dtype).double() @ w.double() + bias.double()).to(dtype)
    ref_err = maxabs(pipe, ref)
    args = (x.to(DEV), w.to(DEV), bias.to(DEV), 0, None, gamma.to(DEV),
            beta.to(DEV), EPS)
    y = ext.gemm(*args) if M == 1 else ext.gemm_skinny(*args)
    k_err = maxabs(y, ref)
    print(f"fused_ln_gemm M={M} K={K} {dtype} ({offset},{std}): kernel "
          f"{k_err:.3e} unfused-f64-stat pipeline {ref_err:.3e}")
    assert k_err <= 4 * ref_err + 1e-6, (k_err, ref_err)


@pytest.mark.parametrize("offset,std", OFFSETS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("M", [1, 2, 8])
def test_fused_ln_gemm_offset(M, dtype, offset, std):
    check_fused_ln_gemm(M, 768, dtype, offset, std)


@pytest.mark.parametrize("offset,std", [(0.0, 1.0), (256.0, 1.0)])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_fused_ln_gemm_long_row(dtype, offset, std):
    """K = 1280: past the row length the VALU skinny prologue keeps in
    registers between its two passes, so it re-reads the row."""
    check_fused_ln_gemm(2, 1280, dtype, offset, std)


# ---------------------------------------------------------------------------
# dispatch and edge coverage (offset 0)
# ---------------------------------------------------------------------------

def ln_reference(x, dy, gamma, beta):
    """float64 layer_norm fwd + autograd bwd on the CPU."""
    D = x.shape[-1]
    xr = x.double().requires_grad_(True)
    gr = gamma.double().requires_grad_(True)
    br = beta.double().requires_grad_(True)
    y = F.layer_norm(xr, (D,), gr, br, EPS)
    y.backward(dy.double())
    return y.detach(), xr.grad, gr.grad, br.grad


def assert_ln(tag, x, dy, x_dev, dy_dev, dtype):
    """ln_fwd + ln_bwd on the given device tensors vs float64; returns the
    kernel outputs."""
    D = x.shape[-1]
    gamma, beta = affine(D)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    y, mean, invstd = ext.ln_fwd(x_dev, gd, bd, EPS)
    assert_stats(tag, mean, invstd, x.double())
    y64, dx64, dg64, db64 = ln_reference(x, dy, gamma, beta)
    dx, dgamma, dbeta = ext.ln_bwd(x_dev, dy_dev, gd, mean, invstd)
    errs = (relerr(y, y64), relerr(dx, dx64), relerr(dgamma, dg64),
            relerr(dbeta, db64))
    print(f"{tag}: relerr y {errs[0]:.3e} dx {errs[1]:.3e} "
          f"dgamma {errs[2]:.3e} dbeta {errs[3]:.3e}")
    assert errs[0] < TOL[dtype] * 2
    assert errs[1] < TOL[dtype] * 4
    assert errs[2] < TOL[dtype] * 4
    assert errs[3] < TOL[dtype] * 4
    return y, mean, invstd, dx, dgamma, dbeta


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("rows,D", [
    (64, 770),    # ragged: scalar fwd, scalar bwd with atomic dgamma/dbeta
    (64, 1001),   # ragged and odd
    (64, 4096),   # fp32: PK=4 fwd, scalar dx + vector column kernel
    (64, 4100),   # fp32: past 4*256 packs -> scalar fwd, column kernel;
                  # bf16: ragged
    (64, 8200),   # both dtypes past the vector fwd; 9 / 5 column blocks
    (1, 768),     # a single row
    (300, 64),    # gpb=16 (8 for bf16), many rows per iteration, rslices > 1
    (3, 1280),    # rslices = 1: single writer; two channel blocks in fp32
])
def test_ln_fwd_bwd_dispatch(rows, D, dtype):
    x = offset_rows(rows, D, 0.0, 1.0, dtype)
    dy = torch.randn(rows, D, generator=_gen(16)).to(dtype)
    tag = f"ln rows={rows} D={D} {dtype}"
    xd, dyd = x.to(DEV), dy.to(DEV)
    _, _, _, dx, dgamma, dbeta = assert_ln(tag, x, dy, xd, dyd, dtype)
    # second call: the atomic path accumulates into a buffer the binding
    # must zero each time. Its adds commute only up to fp32 rounding, so
    # "equal" is up to summation order: rows * 2^-23 * sum |term| per column
    gamma, beta = affine(D)
    y2, mean2, invstd2 = ext.ln_fwd(xd, gamma.to(DEV), beta.to(DEV), EPS)
    dx2, dgamma2, dbeta2 = ext.ln_bwd(xd, dyd, gamma.to(DEV), mean2, invstd2)
    assert torch.equal(dx2, dx)
    xhat = F.layer_norm(x.double(), (D,), None, None, EPS)
    ulp = rows * 2.0 ** -23
    tol_g = ulp * (dy.double() * xhat).abs().sum(0) + 1e-30
    tol_b = ulp * dy.double().abs().sum(0) + 1e-30
    assert ((dgamma2 - dgamma).abs().double().cpu() <= tol_g).all()
    assert ((dbeta2 - dbeta).abs().double().cpu() <= tol_b).all()


def misaligned(t):
    """The same values at a base one element past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=DEV)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 != 0 and v.is_contiguous()
    return v


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("which", ["x", "dy"])
def test_ln_misaligned_base(which, dtype):
    """x off a 16-byte boundary: scalar fwd and scalar/atomic bwd; dy alone
    off it: vector fwd, scalar/atomic bwd. Both must match float64 and the
    aligned call."""
    rows, D = 64, 768
    x = offset_rows(rows, D, 0.0, 1.0, dtype)
    dy = torch.randn(rows, D, generator=_gen(16)).to(dtype)
    xd, dyd = x.to(DEV), dy.to(DEV)
    base = assert_ln(f"ln aligned {dtype}", x, dy, xd, dyd, dtype)
    xm = misaligned(xd) if which == "x" else xd
    dym = misaligned(dyd) if which == "dy" else dyd
    got = assert_ln(f"ln misaligned {which} {dtype}", x, dy, xm, dym, dtype)
    # (mean / invstd of both calls are already held to float64 above)
    for name, i, k in (("y", 0, 2), ("dx", 3, 4), ("dgamma", 4, 4),
                       ("dbeta", 5, 4)):
        assert relerr(got[i], base[i]) < TOL[dtype] * k, name


def bn_reference(x, dy, gamma, beta):
    C = x.shape[-1]
    xr = x.double().requires_grad_(True)
    gr = gamma.double().requires_grad_(True)
    br = beta.double().requires_grad_(True)
    xf = xr.reshape(-1, C)
    m = xf.mean(0)
    var = ((xf - m) ** 2).mean(0)
    y = ((xf - m) * (var + EPS).rsqrt() * gr + br).reshape(x.shape)
    y.backward(dy.double())
    return y.detach(), xr.grad, gr.grad, br.grad


@pytest.mark.parametrize("dtype,C,mis", [
    (F32, 30, False),    # scalar stats / apply / bwd, atomics into zeros
    (F32, 264, False),   # vector path, channel block wider than 256
    (F32, 64, True),     # misaligned x: every kernel falls to scalar
    (BF16, 64, True),
], ids=["fp32-C30", "fp32-C264", "fp32-C64-misaligned", "bf16-C64-misaligned"])
def test_bn_fwd_bwd_dispatch(dtype, C, mis):
    shape = (8, 16, 16, C)
    x = offset_nhwc(shape, 0.0, 1.0, dtype)
    dy = torch.randn(*shape, generator=_gen(17)).to(dtype)
    gamma, beta = affine(C)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    xd = misaligned(x.to(DEV)) if mis else x.to(DEV)
    dyd = dy.to(DEV)
    tag = f"bn C={C} {dtype} misaligned={mis}"
    y, mean, invstd = ext.bn_fwd_train(xd, gd, bd, None, None, 0.1, EPS, False,
                                       0.0, 0, None)
    assert_stats(tag, mean, invstd, x.double().reshape(-1, C).t())
    y64, dx64, dg64, db64 = bn_reference(x, dy, gamma, beta)
    dx, dgamma, dbeta = ext.bn_bwd(xd, dyd, gd, mean, invstd, None, 1.0)
    errs = (relerr(y, y64), relerr(dx, dx64), relerr(dgamma, dg64),
            relerr(dbeta, db64))
    print(f"{tag}: relerr y {errs[0]:.3e} dx {errs[1]:.3e} "
          f"dgamma {errs[2]:.3e} dbeta {errs[3]:.3e}")
    assert errs[0] < TOL[dtype] * 2
    assert errs[1] < TOL[dtype] * 4
    assert errs[2] < TOL[dtype] * 4
    assert errs[3] < TOL[dtype] * 4


@pytest.mark.parametrize("offset,std", [(0.0, 1.0), (64.0, 1.0)])
@pytest.mark.parametrize("momentum", [0.1, 1.0])
@pytest.mark.parametrize("dtype,C", [(F32, 64), (BF16, 64), (F32, 30)],
                         ids=["fp32-C64", "bf16-C64", "fp32-C30"])
def test_bn_running_stats(dtype, C, momentum, offset, std):
    """The running-stat update fused into the finalize kernel: momentum
    blend and the unbiased n/(n-1) factor, over two steps, against
    torch.nn.functional.batch_norm(training=True) in float64.

    Bounds: 1e-5 relative on rvar (fp32 rounding of a handful of
    operations; a biased variance would be off by 1/2047 = 4.9e-4). rmean is
    judged on the scale of the data, max(|rmean|, std): 1e-5 of that, plus
    the 2e-3 * std the batch mean itself is allowed in the offset variant.
    """
    shape = (8, 16, 16, C)
    gamma, beta = affine(C)
    g = _gen(18)
    rm0 = torch.randn(C, generator=g) * 0.5
    rv0 = torch.rand(C, generator=g) + 0.5
    rm, rv = rm0.to(DEV), rv0.to(DEV)
    rm64, rv64 = rm0.double(), rv0.double()
    for step in range(2):
        x = offset_nhwc(shape, offset, std, dtype, seed=19 + step)
        ext.bn_fwd_train(x.to(DEV), gamma.to(DEV), beta.to(DEV), rm, rv,
                         momentum, EPS, False, 0.0, 0, None)
        F.batch_norm(x.double().permute(0, 3, 1, 2), rm64, rv64,
                     gamma.double(), beta.double(), True, momentum, EPS)
        std64 = x.double().reshape(-1, C).std(0)
        e_rv = ((rv.double().cpu() - rv64).abs() / rv64).max().item()
        scale = torch.maximum(rm64.abs(), std64)
        d_rm = (rm.double().cpu() - rm64).abs()
        slack = 1e-5 * scale + (MEAN_BOUND * std64 if offset else 0.0)
        print(f"bn running C={C} {dtype} mom={momentum} ({offset},{std}) "
              f"step {step}: rvar rel {e_rv:.3e} rmean worst/allowed "
              f"{(d_rm / slack).max().item():.3e}")
        assert e_rv <= 1e-5, e_rv
        assert (d_rm <= slack).all()
