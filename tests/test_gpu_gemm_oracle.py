"""GEMM family on the GPU against the float64 oracle (gemm_oracle.py).

Every case runs from guard-banded operands: contiguous views into larger
NaN-filled buffers, 16-byte aligned or, for the unaligned routes, an odd
element count in. Layer 1 must equal the exact integer reference bit for
bit, layer 2 must stay within the element-wise bound, a NaN anywhere means
a read outside an operand reached an output, and a second call must return
the same bits. The id names the route; each test prints its worst
err / bound. The binding checks at the end raise before any launch.
"""

import json
import os
import subprocess
import sys

import pytest
import torch

import gemm_oracle as go

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from tnn_amd import _C
    ext = _C.ext()

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32


def call(c, args):
    a, b, bias, act, resid, g, be = args
    if c.entry == "gemm":
        if c.ln:
            return ext.gemm(a, b, bias, act, resid, g, be, go.LN_EPS)
        return ext.gemm(a, b, bias, act, resid)
    if c.entry == "gemm_skinny":
        return ext.gemm_skinny(a, b, bias, act, resid, g, be, go.LN_EPS)
    if c.entry == "gemm_nt":
        return ext.gemm_nt(a, b)
    if c.entry == "gemm_tn":
        return ext.gemm_tn(a, b, c.out_in_dt)
    return ext.bmm(a, b)


def same_bits(x, y):
    it = torch.int16 if x.dtype == BF16 else torch.int32
    return x.dtype == y.dtype and torch.equal(x.view(it), y.view(it))


def run_exact(c):
    """{epilogue: (largest difference from the exact reference, repeat is
    bit-identical)} of a layer-1 case"""
    out = {}
    for ep in c.eps:
        args = go.device_args(c, go.inputs1(c), DEV, ep, layer=1)
        y1 = call(c, args)
        y2 = call(c, args)
        out[ep] = (go.check_exact(y1, c, ep), same_bits(y1, y2))
    return out


def run_bound(c):
    """(worst err / bound, repeat is bit-identical) of a layer-2 case"""
    args = go.device_args(c, go.inputs2(c), DEV, layer=2)
    y1 = call(c, args)
    y2 = call(c, args)
    assert y1.dtype == c.out_dtype
    return go.check_bound(y1, c), same_bits(y1, y2)


def assert_exact(c, res):
    print(f"{c.id}: " + "  ".join(f"{ep} diff {d:g}" for ep, (d, _) in
                                  res.items()))
    for ep, (d, rep) in res.items():
        assert d == 0.0, f"{c.id} {ep}: differs from the exact reference " \
                         f"by up to {d}"
        assert rep, f"{c.id} {ep}: second call returned other bits"


def assert_bound(c, res):
    ratio, rep = res
    print(f"{c.id}: worst err / bound {ratio:.3f}")
    assert ratio <= 1.0, f"{c.id}: {ratio:.3f} bounds from float64"
    assert rep, f"{c.id}: second call returned other bits"


@pytest.mark.parametrize("c", go.cases_for(1), ids=lambda c: c.id)
def test_exact(c):
    assert_exact(c, run_exact(c))


@pytest.mark.parametrize("c", go.cases_for(2), ids=lambda c: c.id)
def test_bound(c):
    assert_bound(c, run_bound(c))


# bf16 16x16-tile routes, reachable only with TNN_GEMM32=0 (read once per
# process): one fresh child runs all of them
def gemm16_results():
    out = {}
    for c in go.GEMM16_CASES:
        out[c.id] = {"exact": run_exact(c) if 1 in c.layers else None,
                     "bound": run_bound(c) if 2 in c.layers else None}
    return out


def test_gemm16_routes_fresh_process():
    here = os.path.dirname(os.path.abspath(__file__))
    child = ("import sys, json; sys.path[:0] = [%r, %r]; "
             "import test_gpu_gemm_oracle as t; "
             "print('RES ' + json.dumps(t.gemm16_results()))"
             % (os.path.dirname(here), here))
    r = subprocess.run([sys.executable, "-c", child],
                       env=dict(os.environ, TNN_GEMM32="0"),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("RES ")][-1]
    res = json.loads(line[4:])
    assert set(res) == {c.id for c in go.GEMM16_CASES}
    for c in go.GEMM16_CASES:
        if 1 in c.layers:
            assert_exact(c, {ep: tuple(v)
                             for ep, v in res[c.id]["exact"].items()})
        if 2 in c.layers:
            assert_bound(c, tuple(res[c.id]["bound"]))


# ---------------------------------------------------------------------------
# binding checks: all of these raise before any launch
# ---------------------------------------------------------------------------

def _t(*shape, dtype=F32, device=DEV):
    return torch.ones(*shape, dtype=dtype, device=device)


@pytest.mark.parametrize("fn", ["gemm_nt", "gemm_tn"])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_nt_tn_reject_mixed_dtypes(fn, dtype):
    other = BF16 if dtype == F32 else F32
    a, b = _t(64, 64, dtype=dtype), _t(64, 64, dtype=other)
    with pytest.raises(RuntimeError, match=fn + " dtype mismatch: b is"):
        if fn == "gemm_nt":
            ext.gemm_nt(a, b)
        else:
            ext.gemm_tn(a, b, False)


def test_gemm_rejects_bad_ln_arguments():
    K, N = 64, 32
    a, b = _t(1, K), _t(K, N)
    g, be = _t(K), _t(K)
    for bad, name in [(_t(K, device="cpu"), "on GPU|GPU tensor"),
                      (_t(2 * K)[::2], "contiguous"),
                      (_t(K - 1), "contiguous GPU tensor of")]:
        with pytest.raises(RuntimeError, match="ln_gamma.*(%s)" % name):
            ext.gemm(a, b, None, 0, None, bad, be, 1e-5)
        with pytest.raises(RuntimeError, match="ln_beta.*(%s)" % name):
            ext.gemm(a, b, None, 0, None, g, bad, 1e-5)


def test_gemm_rejects_cpu_bias_and_residual():
    a, b = _t(32, 64), _t(64, 32)
    with pytest.raises(RuntimeError, match="bias must be on GPU"):
        ext.gemm(a, b, _t(32, device="cpu"), 0)
    with pytest.raises(RuntimeError, match="residual must be on GPU"):
        ext.gemm(a, b, _t(32), 0, _t(32, 32, device="cpu"))


@pytest.mark.parametrize("dim", ["M", "N", "K"])
def test_empty_operands_raise(dim):
    M, N, K = (0 if dim == d else 8 for d in "MNK")
    calls = {
        "gemm": lambda: ext.gemm(_t(M, K), _t(K, N), None, 0),
        "gemm_ln": lambda: ext.gemm(_t(1, K), _t(K, N), None, 0, None,
                                    _t(K), _t(K), 1e-5),
        "gemm_skinny": lambda: ext.gemm_skinny(_t(M, K), _t(K, N), None, 0),
        "gemm_nt": lambda: ext.gemm_nt(_t(M, K), _t(N, K)),
        "gemm_tn": lambda: ext.gemm_tn(_t(M, K), _t(M, N), False),
        "bmm": lambda: ext.bmm(_t(2, M, K), _t(2, K, N)),
    }
    for name, f in calls.items():
        if name == "gemm_ln" and dim == "M":
            continue        # M is fixed at 1 there
        with pytest.raises(RuntimeError, match="empty operand|1 <= M"):
            f()
    if dim == "M":
        with pytest.raises(RuntimeError, match="empty operand"):
            ext.bmm(_t(0, 8, 8), _t(0, 8, 8))
