"""Gradient sinks: the split reduce of conv wgrad and the slab finalize of BN
backward write dw / db / dgamma / dbeta straight into a caller's buffer
(``conv2d_wgrad_into``, ``bn_bwd(dgamma_out=, dbeta_out=)``), overwriting or
accumulating, and ``GraphedTrainStep`` registers its gradient slabs as such
sinks so autograd no longer adds every gradient to a zeroed buffer.

What must hold, bit for bit (``torch.equal``):
  overwrite   destinations pre-filled with NaN equal ``conv2d_wgrad_bias`` /
              the sums ``bn_bwd`` returns; guard elements around them, carved
              from one larger buffer, keep their value
  accumulate  destinations pre-filled with g0 equal
              ``(g0.float() + g32).to(dtype)``, g32 the fp32-output gradient of
              the same call (same route, same z): one fp32 add, one rounding
The route and z of every case are asserted by name, so a run that took another
kernel does not pass. The switches are read once per process: the default
rule runs in this process, ``TNN_WGRAD_WIDE=2`` (the wide tile wherever
eligible) in one child process.

Which reduce kernel a case takes follows from (n, n_shape, z) by the rule in
``splitk_reduce_launch``; ``_reduce_kernel`` mirrors it, and the test asserts
that the cases cover all three kernels and the "cannot split" fallback. The
1x1 stride-2 shape has M = 256 = one split, so it reduces with z = 1 on
``k_splitk_reduce4``; ``fold_z8`` (M = 2048, z = 8, 18432 outputs) is the case
that reaches ``k_splitk_fold``.

Autograd level: a parameter used twice in one step is written, then
accumulated into: ``(first.to(dtype).float() + second32).to(dtype)``, where
first is the use whose backward runs first. That is the accumulate rule above
applied to the first write, which a buffer of the parameter's dtype cannot
avoid rounding.
"""

import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
GUARD = 8          # elements; keeps both destinations on a group of 4
SENTINEL = 7.0

# name -> ((N, H, W, Cin, Cout, K, stride, pad), input dtype)
CASES = {
    "ragged_kout": ((4, 16, 16, 16, 128, 3, 1, 1), BF),
    "tr_128": ((3, 8, 8, 128, 128, 3, 1, 1), BF),
    "deep_z": ((32, 16, 16, 256, 256, 3, 1, 1), BF),
    "shortcut": ((4, 16, 16, 128, 256, 1, 2, 0), BF),
    "cout10": ((2, 8, 8, 8, 10, 3, 1, 1), BF),
    "fp32_direct": ((2, 8, 8, 16, 16, 3, 1, 1), F32),
    "fold_z8": ((8, 16, 16, 16, 128, 3, 1, 1), BF),
}
# (kernel, z) under the default rule and under TNN_WGRAD_WIDE=2
ROUTES = {
    "auto": {
        "ragged_kout": ("k_conv_wgrad_tr", 4),
        "tr_128": ("k_conv_wgrad_tr", 1),
        "deep_z": ("k_conv_wgrad_tr_wide<db>", 14),
        "shortcut": ("k_conv_wgrad_tr", 1),
        "cout10": ("k_conv_wgrad", 1),
        "fp32_direct": ("k_conv_wgrad_vec", 1),
        "fold_z8": ("k_conv_wgrad_tr", 8),
    },
    "wide": {
        "ragged_kout": ("k_conv_wgrad_tr_wide<db>", 4),
        "tr_128": ("k_conv_wgrad_tr_wide<db>", 1),
        "deep_z": ("k_conv_wgrad_tr_wide<db>", 14),
        "shortcut": ("k_conv_wgrad_tr_wide<db>", 1),
        "cout10": ("k_conv_wgrad", 1),
        "fp32_direct": ("k_conv_wgrad_vec", 1),
        "fold_z8": ("k_conv_wgrad_tr_wide<db>", 8),
    },
}
SWITCHES = ("TNN_WGRAD_WIDE", "TNN_WGRAD_WIDE_BUF", "TNN_WGRAD_SPLITS",
            "TNN_WGRAD_WAVES")


def _reduce_kernel(n, n_shape, z):
    """The rule of splitk_reduce_launch."""
    if n % 4 == 0 and n_shape % 4 == 0 and n_shape < 4 * 32768 and z >= 8:
        return "k_splitk_fold"
    return "k_splitk_reduce4" if n % 4 == 0 else "k_splitk_reduce"


def _inputs(case, dtype, seed):
    N, H, W, Ci, Co, K, S, P = case
    g = torch.Generator().manual_seed(seed)
    OH = (H + 2 * P - K) // S + 1
    OW = (W + 2 * P - K) // S + 1
    x = torch.randn(N, H, W, Ci, generator=g).bfloat16().to(dtype)
    dy = torch.randn(N, OH, OW, Co, generator=g).bfloat16().to(dtype)
    return x.to(DEV), dy.to(DEV)


def _carve(shape_w, Co, dtype, guard, fill_w, fill_b):
    """dw and db destinations inside one buffer, guards on both sides of
    each; returns (buffer, dw view, db view, guard mask)."""
    nw = 1
    for d in shape_w:
        nw *= d
    total = guard + nw + guard + Co + guard
    buf = torch.full((total,), SENTINEL, dtype=dtype, device=DEV)
    mask = torch.ones(total, dtype=torch.bool, device=DEV)
    a, b = guard, guard + nw + guard
    dw = buf[a:a + nw].view(shape_w)
    db = buf[b:b + Co]
    mask[a:a + nw] = False
    mask[b:b + Co] = False
    for dst, fill in ((dw, fill_w), (db, fill_b)):
        if isinstance(fill, float):
            dst.fill_(fill)
        else:
            dst.copy_(fill)
    return buf, dw, db, mask


def _same(a, b):
    return bool(torch.equal(a, b)), int((a != b).sum().item())


def _run_native():
    """Every case x output dtype: route, overwrite, no-bias, accumulate."""
    from tnn_amd import _C
    ext = _C.ext()
    out = {}
    for name, (case, in_dt) in CASES.items():
        N, H, W, Ci, Co, K, S, P = case
        x, dy = _inputs(case, in_dt, sum(map(ord, name)))
        args = (x, dy, K, K, S, S, P, P)
        kernel, z = ext.conv2d_wgrad_route(*args)
        res = {"route": (kernel, int(z)),
               "reduce": _reduce_kernel((K * K * Ci + 1) * Co, K * K * Ci * Co,
                                        int(z))}
        dw32, db32 = ext.conv2d_wgrad_bias(*args, False)
        shape_w = (K, K, Ci, Co)
        nan = float("nan")
        g = torch.Generator().manual_seed(5)
        for out_dt in ([F32] if in_dt == F32 else [BF, F32]):
            tag = "bf16" if out_dt == BF else "fp32"
            ref_w, ref_b = ext.conv2d_wgrad_bias(*args, out_dt == in_dt)
            assert ref_w.dtype == out_dt
            guards = [GUARD] + ([3] if name == "tr_128" else [])
            for guard in guards:
                key = tag if guard == GUARD else tag + "_misaligned"
                # overwrite
                buf, dw, db, mask = _carve(shape_w, Co, out_dt, guard, nan, nan)
                ext.conv2d_wgrad_into(*args, dw, db, False)
                r = {"dw": _same(dw, ref_w), "db": _same(db, ref_b),
                     "guards": bool((buf[mask] == SENTINEL).all())}
                # dw alone
                buf, dw, db, mask = _carve(shape_w, Co, out_dt, guard, nan,
                                           SENTINEL)
                ext.conv2d_wgrad_into(*args, dw)
                r["alone"] = _same(dw, ext.conv2d_wgrad(*args,
                                                        out_dt == in_dt))
                r["alone_guards"] = bool((buf[mask] == SENTINEL).all()
                                         and (db == SENTINEL).all())
                # accumulate
                g0w = torch.randn(shape_w, generator=g).to(out_dt).to(DEV)
                g0b = torch.randn(Co, generator=g).to(out_dt).to(DEV)
                buf, dw, db, mask = _carve(shape_w, Co, out_dt, guard, g0w,
                                           g0b)
                ext.conv2d_wgrad_into(*args, dw, db, True)
                r["acc_dw"] = _same(dw, (g0w.float() + dw32).to(out_dt))
                r["acc_db"] = _same(db, (g0b.float() + db32).to(out_dt))
                r["acc_guards"] = bool((buf[mask] == SENTINEL).all())
                res[key] = r
        out[name] = res
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def native():
    for k in SWITCHES:
        assert k not in os.environ, f"{k} set: this module expects defaults"
    return _run_native()


@pytest.fixture(scope="module")
def native_wide(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("grad_sink") / "wide.pt")
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env["TNN_WGRAD_WIDE"] = "2"
    subprocess.run([sys.executable, os.path.abspath(__file__), "native", path],
                   env=env, check=True, timeout=120)
    return torch.load(path)


def _check_case(got, want_route):
    print(got["route"], got["reduce"])
    assert got["route"] == want_route
    for key, r in got.items():
        if key in ("route", "reduce"):
            continue
        print(key, r)
        for what in ("dw", "db", "alone", "acc_dw", "acc_db"):
            assert r[what][0], (key, what, f"{r[what][1]} elements differ")
        for what in ("guards", "alone_guards", "acc_guards"):
            assert r[what], (key, what)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_wgrad_into_default_routes(name, native):
    _check_case(native[name], ROUTES["auto"][name])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_wgrad_into_wide_routes(name, native_wide):
    _check_case(native_wide[name], ROUTES["wide"][name])


@pytest.mark.gpu
def test_cases_cover_every_reduce_kernel(native):
    kernels = {name: got["reduce"] for name, got in native.items()}
    print(kernels)
    assert kernels["deep_z"] == "k_splitk_reduce4"
    assert kernels["fold_z8"] == "k_splitk_fold"
    assert kernels["cout10"] == "k_splitk_reduce"
    assert "bf16_misaligned" in native["tr_128"]


# ---- BN backward -----------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("rows_shape,C", [((7, 11), 16), ((4, 4, 4), 128)])
@pytest.mark.parametrize("dtype", [BF, F32])
def test_bn_bwd_sinks(rows_shape, C, dtype):
    from tnn_amd import _C
    ext = _C.ext()
    g = torch.Generator().manual_seed(C)
    x = torch.randn(*rows_shape, C, generator=g).to(dtype).to(DEV)
    dy = torch.randn(*rows_shape, C, generator=g).to(dtype).to(DEV)
    gamma = torch.randn(C, generator=g).to(DEV)
    mean = (0.1 * torch.randn(C, generator=g)).to(DEV)
    invstd = (torch.rand(C, generator=g) + 0.5).to(DEV)
    assert ext.bn_bwd_takes_sink(x, dy), "slab path expected"
    dx0, dgamma0, dbeta0 = ext.bn_bwd(x, dy, gamma, mean, invstd, None, 1.0)

    def carve(fill_g, fill_b):
        buf = torch.full((3 * GUARD + 2 * C,), SENTINEL, device=DEV)
        dg = buf[GUARD:GUARD + C]
        db = buf[2 * GUARD + C:2 * GUARD + 2 * C]
        dg.copy_(fill_g)
        db.copy_(fill_b)
        return buf, dg, db

    def guards_ok(buf):
        return bool((buf[:GUARD] == SENTINEL).all()
                    and (buf[GUARD + C:2 * GUARD + C] == SENTINEL).all()
                    and (buf[2 * GUARD + 2 * C:] == SENTINEL).all())

    nan = torch.full((C,), float("nan"), device=DEV)
    buf, dg, db = carve(nan, nan)
    dx1, dgamma1, dbeta1 = ext.bn_bwd(x, dy, gamma, mean, invstd, None, 1.0,
                                      dgamma_out=dg, dbeta_out=db)
    assert torch.equal(dx1, dx0)
    assert torch.equal(dgamma1, dgamma0) and torch.equal(dbeta1, dbeta0)
    assert torch.equal(dg, dgamma0) and torch.equal(db, dbeta0)
    assert guards_ok(buf)

    g0g = torch.randn(C, generator=g).to(DEV)
    g0b = torch.randn(C, generator=g).to(DEV)
    buf, dg, db = carve(g0g, g0b)
    dx2, _, _ = ext.bn_bwd(x, dy, gamma, mean, invstd, None, 1.0,
                           dgamma_out=dg, dbeta_out=db, accumulate=True)
    assert torch.equal(dx2, dx0)
    assert torch.equal(dg, g0g + dgamma0) and torch.equal(db, g0b + dbeta0)
    assert guards_ok(buf)


# ---- binding checks --------------------------------------------------------

@pytest.mark.gpu
def test_binding_checks():
    from tnn_amd import _C
    ext = _C.ext()
    x = torch.randn(2, 8, 8, 16, device=DEV).bfloat16()
    dy = torch.randn(2, 8, 8, 32, device=DEV).bfloat16()
    args = (x, dy, 3, 3, 1, 1, 1, 1)

    def dw(dtype=BF, shape=(3, 3, 16, 32)):
        return torch.zeros(shape, dtype=dtype, device=DEV)

    def db(dtype=BF, n=32):
        return torch.zeros(n, dtype=dtype, device=DEV)

    ext.conv2d_wgrad_into(*args, dw(), db(), False)          # the good call
    with pytest.raises(RuntimeError, match="dw_out"):
        ext.conv2d_wgrad_into(*args, dw(torch.float16), db(), False)
    with pytest.raises(RuntimeError, match="db_out"):
        ext.conv2d_wgrad_into(*args, dw(), db(F32), False)   # mixed dtypes
    with pytest.raises(RuntimeError, match="shape"):
        ext.conv2d_wgrad_into(*args, dw(shape=(3, 3, 32, 16)), db(), False)
    with pytest.raises(RuntimeError, match="shape"):
        ext.conv2d_wgrad_into(*args, dw(), db(n=16), False)
    with pytest.raises(RuntimeError, match="contiguous"):
        ext.conv2d_wgrad_into(
            *args, dw(shape=(3, 3, 32, 16)).transpose(2, 3), db(), False)
    with pytest.raises(RuntimeError, match="GPU"):
        ext.conv2d_wgrad_into(*args, dw().cpu(), db(), False)

    C = 32
    gamma = torch.ones(C, device=DEV)
    mean = torch.zeros(C, device=DEV)
    bn = (dy, dy, gamma, mean, gamma, None, 1.0)
    good = torch.zeros(C, device=DEV)
    ext.bn_bwd(*bn, dgamma_out=good, dbeta_out=good.clone())
    with pytest.raises(RuntimeError, match="dgamma_out"):
        ext.bn_bwd(*bn, dgamma_out=good.bfloat16(), dbeta_out=good)
    with pytest.raises(RuntimeError, match="shape"):
        ext.bn_bwd(*bn, dgamma_out=good, dbeta_out=torch.zeros(C + 1,
                                                              device=DEV))
    with pytest.raises(RuntimeError, match="contiguous"):
        ext.bn_bwd(*bn, dgamma_out=torch.zeros(C, 2, device=DEV)[:, 0],
                   dbeta_out=good)
    with pytest.raises(RuntimeError, match="go together"):
        ext.bn_bwd(*bn, dgamma_out=good)


# ---- autograd level --------------------------------------------------------

class _Net(torch.nn.Module):
    """Conv(3->16) - ReLU - BN - [Conv(16->16) - ReLU, twice] - Conv(16->128)
    - ReLU - BN - pool - dense. No Conv->BN pair is adjacent, so the fused
    conv statistics (atomics) stay out of it."""

    def __init__(self, twice):
        super().__init__()
        from tnn_amd.nn import layers as L
        self.c1 = L.Conv2D(3, 16, (3, 3), (1, 1), (1, 1), name="c1")
        self.bn1 = L.BatchNorm(16, name="bn1")
        self.cd = L.Conv2D(16, 16, (3, 3), (1, 1), (1, 1), name="cd")
        self.c2 = L.Conv2D(16, 128, (3, 3), (1, 1), (1, 1), name="c2")
        self.bn2 = L.BatchNorm(128, name="bn2")
        self.pool = L.AvgPool2D((8, 8))
        self.fc = L.Dense(128, 10, name="fc")
        self.twice = twice
        self.taps = None   # [(input, output)] of the cd applications

    def forward(self, x):
        x = self.bn1(torch.relu(self.c1(x)))
        if self.twice:
            for _ in range(2):
                y = self.cd(x)
                if self.taps is not None:
                    self.taps.append((x, y))
                x = torch.relu(y)
        x = self.bn2(torch.relu(self.c2(x)))
        return self.fc(self.pool(x).flatten(1))


def _net(twice):
    from tnn_amd.nn.layer import cast_compute_dtype
    torch.manual_seed(3)
    m = _Net(twice)
    cast_compute_dtype(m, BF)
    return m.to(DEV).train()


def _batch():
    g = torch.Generator().manual_seed(4)
    x = torch.randn(8, 8, 8, 3, generator=g).bfloat16().to(DEV)
    y = torch.randint(0, 10, (8,), generator=g).to(DEV)
    return x, y


def _eager_grads(sinks_on, tap=False):
    """One forward/backward with zeroed .grad buffers; returns the gradients,
    the per-parameter count of autograd deliveries, and the taps."""
    from tnn_amd.nn import CrossEntropyLoss
    from tnn_amd.ops import functional as Fn
    m = _net(twice=True)
    x, y = _batch()
    deliveries = {}
    for name, p in m.named_parameters():
        p.grad = torch.zeros_like(p)
        deliveries[name] = 0

        def hook(g, name=name):
            # autograd calls the hook with None where the backward handed it
            # nothing for this parameter: not a delivery
            if g is not None:
                deliveries[name] += 1
        p.register_hook(hook)
    dys = []
    if tap:
        m.taps = []
    sinks = Fn.GradSinks(m.parameters()) if sinks_on else None
    Fn.set_grad_sinks(sinks)
    try:
        loss = CrossEntropyLoss()(m(x), y)
        if tap:
            for _, out in m.taps:
                out.register_hook(lambda g: dys.append(g.clone()))
        loss.backward()
    finally:
        Fn.set_grad_sinks(None)
    torch.cuda.synchronize()
    grads = {n: p.grad.clone() for n, p in m.named_parameters()}
    taps = [(a.detach(), None) for a, _ in m.taps] if tap else None
    return grads, deliveries, taps, dys


FALLBACKS = {"c1.weight", "fc.weight", "fc.bias"}   # stem dw, the dense layer


@pytest.mark.gpu
def test_autograd_sinks_match_autograd_adds():
    from tnn_amd import _C
    ext = _C.ext()
    off1, dlv_off, _, _ = _eager_grads(False)
    off2, _, _, _ = _eager_grads(False)
    # premise: the sink-off gradients are reproducible bit for bit
    for n in off1:
        assert torch.equal(off1[n], off2[n]), f"premise: {n} not reproducible"
    assert all(v == 1 for n, v in dlv_off.items() if not n.startswith("cd.")), \
        dlv_off
    on, dlv_on, taps, dys = _eager_grads(True, tap=True)
    print(dlv_on)
    for n in on:
        if n.startswith("cd."):
            continue
        assert torch.equal(on[n], off1[n]), n
    # autograd delivers a gradient only for the declared fallbacks
    assert {n for n, v in dlv_on.items() if v} == FALLBACKS, dlv_on
    assert all(dlv_on[n] == 1 for n in FALLBACKS)
    # the parameter used twice: written by the backward that runs first (the
    # second application), accumulated into by the other
    assert len(taps) == 2 and len(dys) == 2
    (x_a, _), (x_b, _) = taps        # forward order
    dy_b, dy_a = dys                 # backward order
    a32 = ext.conv2d_wgrad_bias(x_a, dy_a.contiguous(), 3, 3, 1, 1, 1, 1, False)
    b32 = ext.conv2d_wgrad_bias(x_b, dy_b.contiguous(), 3, 3, 1, 1, 1, 1, False)
    for n, first, second in (("cd.weight", b32[0], a32[0]),
                             ("cd.bias", b32[1], a32[1])):
        want = (first.to(BF).float() + second).to(BF)
        assert torch.equal(on[n], want), n


def _graphed_params(path=None):
    from tnn_amd.nn import AdamW, CrossEntropyLoss
    from tnn_amd.utils.graphstep import GraphedTrainStep
    m = _net(twice=False)
    x, y = _batch()
    opt = AdamW(m.parameters(), lr=1e-2)
    g = GraphedTrainStep(m, CrossEntropyLoss(), opt, x, y, warmup=2)
    for _ in range(3):
        loss = g()
    torch.cuda.synchronize()
    out = {"loss": loss.float().cpu(),
           "written": None if g._sink_written is None
           else len(g._sink_written),
           "fills": None if g._zero_views is None else len(g._zero_views),
           "state": {k: v.cpu() for k, v in m.state_dict().items()}}
    if path:
        torch.save(out, path)
    return out


@pytest.mark.gpu
def test_graphed_step_sinks_match_sinks_off(tmp_path):
    assert os.environ.get("TNN_GRAD_SINK", "1") != "0"
    on = _graphed_params()
    path = str(tmp_path / "off.pt")
    subprocess.run([sys.executable, os.path.abspath(__file__), "graphed", path],
                   env=dict(os.environ, TNN_GRAD_SINK="0"), check=True,
                   timeout=120)
    off = torch.load(path)
    print("on:", on["written"], on["fills"], "off:", off["written"],
          off["fills"], "loss", on["loss"].item(), off["loss"].item())
    assert off["written"] is None and off["fills"] is None
    # 3 conv + 4 BN parameters are sunk (c1.bias, c2.*, bn1.*, bn2.*); the
    # fills zero the rest: the fallbacks, and cd, which this model never uses
    assert on["written"] == 7
    assert on["fills"] >= 1
    for k in on["state"]:
        assert torch.equal(on["state"][k], off["state"][k]), k
    assert torch.equal(on["loss"], off["loss"])


@pytest.mark.gpu
def test_graphed_step_accumulates_twice_used_parameter():
    """Accumulation under capture and replay: with lr = 0 the parameters stay
    put, so every execution of the step, the replays included, must leave in
    p.grad exactly what one eager backward with the sinks on leaves, for the
    twice-applied conv too (overwrite by one use, accumulate by the other).
    A replay that accumulated into the previous step's gradient, or that
    overwrote twice, does not pass."""
    from tnn_amd.nn import AdamW, CrossEntropyLoss
    from tnn_amd.utils.graphstep import GraphedTrainStep
    eager, _, _, _ = _eager_grads(True)
    m = _net(twice=True)
    x, y = _batch()
    opt = AdamW(m.parameters(), lr=0.0)
    g = GraphedTrainStep(m, CrossEntropyLoss(), opt, x, y, warmup=2)
    for _ in range(3):
        g()
    torch.cuda.synchronize()
    assert g._sink_written is not None and len(g._sink_written) == 9
    for n, p in m.named_parameters():
        assert torch.equal(p.grad, eager[n]), n


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    if sys.argv[1] == "native":
        torch.save(_run_native(), sys.argv[2])
    else:
        _graphed_params(sys.argv[2])
