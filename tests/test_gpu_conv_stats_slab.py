"""Conv forward fused statistics as slab partials: every block of the
DMA-staged forward kernels stores one ``[2][BN]`` partial (sum, sum of squares
of its tile of y) into ``partials[m-tile][2][Cout]`` with plain stores, and a
fold in a fixed order sums the m-tiles: ``ext.conv2d_fwd_stats`` returns the
folded ``[2, Cout]``, ``ext.conv2d_fwd_partials`` the partials, which
``bn_fwd_train(precomp=...)`` folds inside its finalize kernel. No atomics, so
two calls give the same bits, which the atomic form could not promise.

Checks, per case and route:
  - float (non-integer) inputs, two calls: ``torch.equal`` statistics
  - statistics against a float64 sum of the returned y. The kernel sums the
    fp32 accumulator v, y is v rounded to bf16 (|v - y| <= 2^-9 |v|, taken as
    2^-8 |y|), and an fp32 sum of M terms is off by at most M 2^-24 of the sum
    of magnitudes per addition order (taken as M 2^-23), so
        |sum   - sum64(y)|   <= (2^-8 + M 2^-23) sum64|y|
        |sumsq - sum64(y^2)| <= (2^-7 + 2^-16 + M 2^-23) sum64(y^2)
    (|v^2 - y^2| <= |v - y| (|v| + |y|)); for fp32 y = v and only the
    summation term is left
  - ``bn_fwd_train`` fed the partials equals ``bn_fwd_train`` fed the folded
    ``[2, C]`` bit for bit: y, mean, invstd and both running statistics
  - the route is asserted by name; the default rule runs in this process,
    ``TNN_CONV_WIDE=2`` (the wide tile wherever eligible) in one child

The statistics come from the DMA-staged kernels only, which need power-of-two
extents. ``(2,9,9,16,64,3,1,1)`` (M = 162) therefore takes the plain route and
returns no statistics, before this change as after it: the case checks
exactly that (empty statistics, y equal to ``conv2d_fwd``), and
``(3,8,8,16,64,3,1,1)`` (M = 192: one full and one ragged m-tile, one narrow
n-tile) is the eligible shape with a ragged m-tile.
"""

import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32

# name -> ((N, H, W, Cin, Cout, K, stride, pad), dtype)
CASES = {
    "m162_ineligible": ((2, 9, 9, 16, 64, 3, 1, 1), BF),
    "ragged_mtile": ((3, 8, 8, 16, 64, 3, 1, 1), BF),
    "cout128": ((2, 16, 16, 128, 128, 3, 1, 1), BF),
    "cout256": ((1, 8, 8, 256, 256, 3, 1, 1), BF),
    "k4608": ((1, 8, 8, 512, 512, 3, 1, 1), BF),
    "fp32_db": ((2, 8, 8, 16, 32, 3, 1, 1), F32),
}
ROUTES = {
    "auto": {"m162_ineligible": "k_conv_fwd", "ragged_mtile": "k_conv_fwd_db",
             "cout128": "k_conv_fwd_db", "cout256": "k_conv_fwd_db",
             "k4608": "k_conv_fwd_sb", "fp32_db": "k_conv_fwd_db"},
    "wide": {"m162_ineligible": "k_conv_fwd", "ragged_mtile": "k_conv_fwd_db",
             "cout128": "k_conv_fwd_sb_wide", "cout256": "k_conv_fwd_db_wide",
             "k4608": "k_conv_fwd_db_wide", "fp32_db": "k_conv_fwd_db"},
}
SWITCHES = ("TNN_CONV_WIDE", "TNN_CONV_WIDE_BUF", "TNN_FWD_DB", "TNN_DB_MAXK")


def _inputs(case, dtype, seed):
    N, H, W, Ci, Co, K, S, P = case
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, H, W, Ci, generator=g).bfloat16().to(dtype)
    w = (torch.randn(K, K, Ci, Co, generator=g) / (K * Ci ** 0.5)) \
        .bfloat16().to(dtype)
    b = torch.randn(Co, generator=g).bfloat16().to(dtype)
    return x.to(DEV), w.to(DEV), b.to(DEV)


def _run_all():
    from tnn_amd import _C
    ext = _C.ext()
    out = {}
    for name, (case, dtype) in CASES.items():
        N, H, W, Ci, Co, K, S, P = case
        x, w, b = _inputs(case, dtype, sum(map(ord, name)))
        s = (S, S, P, P)
        res = {"route": ext.conv2d_fwd_route(x, w, *s, True)}
        y, stats = ext.conv2d_fwd_stats(x, w, b, *s)
        y2, stats2 = ext.conv2d_fwd_stats(x, w, b, *s)
        res["y_plain"] = bool(torch.equal(y, ext.conv2d_fwd(x, w, b, *s,
                                                           False)))
        res["eligible"] = stats.numel() > 0
        if stats.numel():
            yp, part = ext.conv2d_fwd_partials(x, w, b, *s)
            M = y.numel() // Co
            res["shape_ok"] = (tuple(stats.shape) == (2, Co) and
                               tuple(part.shape) == ((M + 127) // 128, 2, Co))
            res["repeat"] = bool(torch.equal(stats, stats2)
                                 and torch.equal(y, y2) and torch.equal(y, yp))
            yd = y.double().reshape(-1, Co)
            rnd = 0.0 if dtype == F32 else 1.0
            sumerr = M * 2.0 ** -23
            e0 = (stats[0].double() - yd.sum(0)).abs()
            b0 = (rnd * 2.0 ** -8 + sumerr) * yd.abs().sum(0)
            e1 = (stats[1].double() - (yd * yd).sum(0)).abs()
            b1 = (rnd * (2.0 ** -7 + 2.0 ** -16) + sumerr) * (yd * yd).sum(0)
            res["sum"] = ((e0 / b0).max().item(), bool((e0 <= b0).all()))
            res["sumsq"] = ((e1 / b1).max().item(), bool((e1 <= b1).all()))
            # bn_fwd_train: partials against the folded [2, C]
            gamma = torch.linspace(0.5, 1.5, Co, device=DEV)
            beta = torch.linspace(-1, 1, Co, device=DEV)
            outs = []
            for pre in (part, stats):
                rm = torch.full((Co,), 0.25, device=DEV)
                rv = torch.full((Co,), 0.75, device=DEV)
                yb, mean, invstd = ext.bn_fwd_train(y, gamma, beta, rm, rv,
                                                    0.1, 1e-5, True, 0.0, 0,
                                                    pre, None)
                outs.append((yb, mean, invstd, rm, rv))
            res["bn"] = [bool(torch.equal(a, c)) for a, c in zip(*outs)]
            res["bn_moved"] = bool((outs[0][3] != 0.25).any())
        out[name] = res
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def auto_out():
    for k in SWITCHES:
        assert k not in os.environ, f"{k} set: this module expects defaults"
    return _run_all()


@pytest.fixture(scope="module")
def wide_out(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("stats_slab") / "wide.pt")
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env["TNN_CONV_WIDE"] = "2"
    subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env,
                   check=True, timeout=120)
    return torch.load(path)


def _check(name, got, route):
    print(name, got)
    assert got["route"] == route
    assert got["y_plain"], "y differs from conv2d_fwd"
    if name == "m162_ineligible":
        assert not got["eligible"]
        return
    assert got["eligible"], "fused-statistics route expected"
    assert got["shape_ok"]
    assert got["repeat"], "two calls differ"
    assert got["sum"][1], f"sum err/bound {got['sum'][0]}"
    assert got["sumsq"][1], f"sumsq err/bound {got['sumsq'][0]}"
    assert all(got["bn"]), ("y, mean, invstd, rmean, rvar", got["bn"])
    assert got["bn_moved"], "running statistics not updated"


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_stats_slab_default_routes(name, auto_out):
    _check(name, auto_out[name], ROUTES["auto"][name])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_stats_slab_wide_routes(name, wide_out):
    _check(name, wide_out[name], ROUTES["wide"][name])


@pytest.mark.gpu
def test_precomp_checks():
    from tnn_amd import _C
    ext = _C.ext()
    C = 32
    x = torch.randn(4, 8, 8, C, device=DEV).bfloat16()
    g, b = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)

    def call(pre):
        return ext.bn_fwd_train(x, g, b, None, None, 0.1, 1e-5, False, 0.0, 0,
                                pre, None)

    call(torch.ones(3, 2, C, device=DEV))
    with pytest.raises(RuntimeError, match="precomputed"):
        call(torch.ones(3, 2, C + 1, device=DEV))
    with pytest.raises(RuntimeError, match="precomputed"):
        call(torch.ones(3, 1, C, device=DEV))
    with pytest.raises(RuntimeError, match="precomp"):
        call(torch.ones(3, 2, C, device=DEV).bfloat16())
    with pytest.raises(RuntimeError, match="precomp"):
        call(torch.ones(3, 2, 2 * C, device=DEV)[:, :, ::2])


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    torch.save(_run_all(), sys.argv[1])
