"""Flash attention kernels against a float64 oracle at ragged lengths.

The grid (attn_oracle.CASES) is S in {1, 17, 63, 64, 65, 127, 128, 129, 191,
200, 257} x D in {64, 128} x causal in {False, True}: below one tile, an
exact tile and one row over, the 4-wave to 8-wave forward switch at 128, one
row into a second 128-row Q block, and a ragged third and fifth KV tile.
B=2 and H=3, so bh / H and bh % H run with a non-power-of-two H.

Every output is compared with float64 torch on the kernel's own bf16 inputs
by  nerr = max over (b, h) of max|x - x64| / rms(x64[b, h])  (lse: max
absolute error), against attn_oracle.BOUND. Those bounds are three times the
worst nerr of a CPU rounding model and are shown by test_attn_oracle_cpu.py
to sit at least 3x (in fact 7.9x) below what any mutant of the reference
produces on these same inputs; see that file's docstring for the figures.
No bound here was taken from a kernel's result. Each test prints the
kernel's nerr next to the rounding model's.
"""

import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_oracle as A  # noqa: E402

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from tnn_amd import _C
    ext = _C.ext()

DEV = "cuda"
B, H = A.B, A.H
BF16 = torch.bfloat16


def _id(case):
    return A.case_id(case[:3]) + ("-kspike" if len(case) > 3 else "")


def run_dense(c):
    """attn_fwd then attn_bwd on BHSD-contiguous copies of the case"""
    q, k, v, do = (t.to(DEV) for t in (c.q, c.k, c.v, c.do))
    o, lse = ext.attn_fwd(q, k, v, c.causal)
    dq, dk, dv = ext.attn_bwd(q, k, v, o, do, lse, c.causal)
    torch.cuda.synchronize()
    return {"o": o, "lse": lse, "dq": dq, "dk": dk, "dv": dv}


def merged(c):
    """the case's q, k, v as one [B, S, 3*H*D] buffer on the GPU"""
    return torch.cat([t.transpose(1, 2).reshape(B, c.S, H * c.D)
                      for t in (c.q, c.k, c.v)], dim=-1).to(DEV)


def head_views(buf, D):
    return tuple(t.unflatten(-1, (H, D)).permute(0, 2, 1, 3)
                 for t in buf.split(H * D, dim=-1))


@pytest.mark.parametrize("case", A.CASES, ids=_id)
def test_fwd_bwd_vs_float64(case):
    c = A.get_case(*case)
    got = run_dense(c)
    c.check(_id(case), got)
    if c.S == 1:
        # one key: P = 1 exactly, so o = v and dv = do bit for bit (dq and
        # dk are zero in float64; check() holds them to the bound relative
        # to the terms that cancel)
        assert torch.equal(got["o"].cpu(), c.v)
        assert torch.equal(got["dv"].cpu(), c.do)


@pytest.mark.parametrize("case", A.KSPIKE_CASES, ids=_id)
def test_spiked_k_backward(case):
    """one K row of the last tile times 8: exp(s - lse) in the backward
    spans the range the forward's rescale path sees"""
    c = A.get_case(*case)
    c.check(_id(case), run_dense(c))


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D", A.D_GRID)
@pytest.mark.parametrize("S", [65, 200])
def test_strided_layouts_vs_float64(S, D, causal):
    """q/k/v as head slices of one merged buffer, dout as a transposed view
    of a BSHD buffer, grads into caller-provided views of one dQKV buffer"""
    c = A.get_case(S, D, causal)
    q, k, v = head_views(merged(c), D)
    assert not q.is_contiguous()
    do = c.do.to(DEV).transpose(1, 2).contiguous().transpose(1, 2)
    assert not do.is_contiguous()
    o, lse = ext.attn_fwd(q, k, v, causal)
    dqkv = torch.zeros(B, S, 3 * H * D, dtype=BF16, device=DEV)
    dq_o, dk_o, dv_o = head_views(dqkv, D)
    ext.attn_bwd(q, k, v, o, do, lse, causal,
                 dq_out=dq_o, dk_out=dk_o, dv_out=dv_o)
    torch.cuda.synchronize()
    c.check(f"strided {A.case_id((S, D, causal))}",
            {"o": o, "lse": lse, "dq": dq_o, "dk": dk_o, "dv": dv_o})


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D", A.D_GRID)
def test_bwd_no_stray_writes(D, causal):
    """grad views in the interior of a larger sentinel-filled buffer: rows
    >= S of the last tile and everything around the views stay untouched"""
    S, ROWS, COLS, SENT = 65, 3, 8, 0x5A5A
    c = A.get_case(S, D, causal)
    q, k, v = head_views(merged(c), D)
    o, lse = ext.attn_fwd(q, k, v, causal)
    W = 3 * H * D
    raw = torch.full((B, S + 2 * ROWS, W + 2 * COLS), SENT, dtype=torch.int16,
                     device=DEV)
    inner = raw.view(BF16)[:, ROWS:ROWS + S, COLS:COLS + W]
    dq_o, dk_o, dv_o = head_views(inner, D)
    ext.attn_bwd(q, k, v, o, c.do.to(DEV), lse, causal,
                 dq_out=dq_o, dk_out=dk_o, dv_out=dv_o)
    torch.cuda.synchronize()
    outside = torch.ones_like(raw, dtype=torch.bool)
    outside[:, ROWS:ROWS + S, COLS:COLS + W] = False
    assert outside.sum().item() == raw.numel() - B * S * W
    assert (raw[outside] == SENT).all()
    c.check(f"sentinel {A.case_id((S, D, causal))}",
            {"dq": dq_o, "dk": dk_o, "dv": dv_o})


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D", A.D_GRID)
def test_bwd_repeatable(D, causal):
    """dK and dV have one writer per element: bit-identical run to run.
    dQ is summed with fp32 atomics: equal within the bound."""
    c = A.get_case(200, D, causal)
    a, b = run_dense(c), run_dense(c)
    assert torch.equal(a["o"], b["o"]) and torch.equal(a["lse"], b["lse"])
    assert torch.equal(a["dk"], b["dk"])
    assert torch.equal(a["dv"], b["dv"])
    e = A.nerr(a["dq"], b["dq"].double().cpu())
    print(f"dq run-to-run nerr {e:.3e} bound {A.BOUND['dq']:.3e}")
    assert e <= A.BOUND["dq"]


def waves4_check():
    """runs in a child process started with TNN_ATTN_WAVES=4: the 4-wave
    forward at lengths the default dispatch gives to the 8-wave form"""
    ok = True
    for S in (129, 200):
        for D in A.D_GRID:
            for causal in (False, True):
                c = A.get_case(S, D, causal)
                q, k, v = (t.to(DEV) for t in (c.q, c.k, c.v))
                o, lse = ext.attn_fwd(q, k, v, causal)
                torch.cuda.synchronize()
                try:
                    c.check(f"waves4 {A.case_id((S, D, causal))}",
                            {"o": o, "lse": lse})
                except AssertionError as e:
                    print(e)
                    ok = False
    return ok


def test_fwd_four_wave_form_at_long_s():
    # the wave count is read once per process, so it needs one of its own
    here = os.path.dirname(os.path.abspath(__file__))
    child = ("import sys; sys.path[:0] = [%r, %r]; "
             "import test_gpu_attention_oracle as t; "
             "print('WAVES4_OK', t.waves4_check())"
             % (os.path.dirname(here), here))
    r = subprocess.run([sys.executable, "-c", child],
                       env=dict(os.environ, TNN_ATTN_WAVES="4"),
                       capture_output=True, text=True, timeout=120)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stderr[-2000:]
    assert "WAVES4_OK True" in r.stdout, r.stdout[-2000:]


@pytest.mark.parametrize("causal", [False, True])
def test_flash_attention_wrapper_grads(causal):
    """flash_attention on transposed views of BSHD leaves"""
    from tnn_amd.ops.flash import flash_attention
    c = A.get_case(65, 64, causal)
    leaves = [t.transpose(1, 2).contiguous().to(DEV).requires_grad_()
              for t in (c.q, c.k, c.v)]
    q, k, v = (t.transpose(1, 2) for t in leaves)
    assert not q.is_contiguous()
    o = flash_attention(q, k, v, causal=causal)
    o.backward(c.do.to(DEV))
    torch.cuda.synchronize()
    dq, dk, dv = (t.grad.transpose(1, 2) for t in leaves)
    c.check(f"flash_attention {A.case_id((65, 64, causal))}",
            {"o": o, "dq": dq, "dk": dk, "dv": dv})


@pytest.mark.parametrize("causal", [False, True])
def test_flash_attention_qkv_wrapper_grads(causal):
    """flash_attention_qkv on one merged [B, S, 3*H*D] leaf"""
    from tnn_amd.ops.flash import flash_attention_qkv
    S, D = 65, 64
    c = A.get_case(S, D, causal)
    qkv = merged(c).requires_grad_()
    o = flash_attention_qkv(qkv, H, causal)
    assert o.shape == (B, S, H * D)
    o.backward(c.do.to(DEV).transpose(1, 2).reshape(B, S, H * D))
    torch.cuda.synchronize()
    dq, dk, dv = head_views(qkv.grad, D)
    c.check(f"flash_attention_qkv {A.case_id((S, D, causal))}",
            {"o": o.unflatten(-1, (H, D)).transpose(1, 2),
             "dq": dq, "dk": dk, "dv": dv})


def test_bindings_reject_mismatched_tensors():
    """Every mismatch here is shaped so that the kernels would still stay
    inside every allocation if a check were missing: longer tensors, wider
    dtypes, and pinned (GPU-visible) host memory for the device checks."""
    S, D = 65, 64
    c = A.get_case(S, D, True)
    q, k, v, do = (t.to(DEV) for t in (c.q, c.k, c.v, c.do))
    o, lse = ext.attn_fwd(q, k, v, True)
    dq0, dk0, dv0 = ext.attn_bwd(q, k, v, o, do, lse, True)   # all valid
    torch.cuda.synchronize()

    def longer(t):          # [B, H, S + 64, D] or [B, H, S + 64]
        pad = list(t.shape)
        pad[2] = 64
        return torch.cat([t, torch.zeros(pad, dtype=t.dtype, device=DEV)], 2)

    def pinned(t):
        return t.cpu().pin_memory()

    def narrow_d(t):        # D = 32: no kernel is instantiated for it
        return t[..., :32].contiguous()

    for name, bad in (("k", longer(k)), ("v", longer(v)),
                      ("k", k.float()), ("v", v.float()),
                      ("k", pinned(k)), ("v", pinned(v))):
        args = dict(q=q, k=k, v=v)
        args[name] = bad
        with pytest.raises(RuntimeError, match=f"attn_fwd: {name} must be"):
            ext.attn_fwd(args["q"], args["k"], args["v"], True)
        with pytest.raises(RuntimeError, match=f"attn_bwd: {name} must be"):
            ext.attn_bwd(args["q"], args["k"], args["v"], o, do, lse, True)
    for fn in (lambda: ext.attn_fwd(q.float(), k.float(), v.float(), True),
               lambda: ext.attn_bwd(q.float(), k.float(), v.float(), o, do,
                                    lse, True)):
        with pytest.raises(RuntimeError, match="flash attention is bf16"):
            fn()
    q32, k32, v32 = narrow_d(q), narrow_d(k), narrow_d(v)
    with pytest.raises(RuntimeError, match="head dim must be 64 or 128"):
        ext.attn_fwd(q32, k32, v32, True)
    with pytest.raises(RuntimeError, match="head dim must be 64 or 128"):
        ext.attn_bwd(q32, k32, v32, narrow_d(o), narrow_d(do), lse, True)
    with pytest.raises(RuntimeError, match=r"q must be \[B,H,S,D\]"):
        ext.attn_bwd(q[0], k[0], v[0], o[0], do[0], lse[0], True)

    lse2 = torch.zeros(B, H, 2 * S, device=DEV)
    lse2[..., ::2] = lse
    for name, bad in (("o", longer(o)), ("o", o.float()), ("o", pinned(o)),
                      ("dout", longer(do)), ("dout", do.float()),
                      ("dout", pinned(do)),
                      ("lse", longer(lse)), ("lse", lse.double()),
                      ("lse", pinned(lse)), ("lse", lse2[..., ::2])):
        args = dict(o=o, dout=do, lse=lse)
        args[name] = bad
        with pytest.raises(RuntimeError, match=f"attn_bwd: {name} must be"):
            ext.attn_bwd(q, k, v, args["o"], args["dout"], args["lse"], True)

    def grads():
        return [torch.zeros_like(q) for _ in range(3)]

    for i, name in enumerate(("dq_out", "dk_out", "dv_out")):
        for make in (longer, torch.Tensor.float, pinned):
            g = grads()
            g[i] = make(g[i])
            with pytest.raises(RuntimeError,
                               match=f"attn_bwd: {name} must be"):
                ext.attn_bwd(q, k, v, o, do, lse, True, dq_out=g[0],
                             dk_out=g[1], dv_out=g[2])
    with pytest.raises(RuntimeError, match="all three grad views or none"):
        ext.attn_bwd(q, k, v, o, do, lse, True, dq_out=grads()[0])

    # nothing above reached a kernel: the valid call still gives what it did
    dq1, dk1, dv1 = ext.attn_bwd(q, k, v, o, do, lse, True)
    torch.cuda.synchronize()
    assert torch.equal(dk1, dk0) and torch.equal(dv1, dv0)
