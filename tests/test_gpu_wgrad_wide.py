"""bf16 conv wgrad on the 128x128 block tile (k_conv_wgrad_tr_wide<db>, <sb>).

The wide kernels share their body with k_conv_wgrad_tr: same k-major images,
same split boundaries for the same split count z, and for every output element
the same chunks, k-steps and MFMA sequence. So with z pinned (TNN_WGRAD_SPLITS)
dw and db must be equal bit for bit between the 128x64 kernel and both wide
forms, fp32 out and bf16 out. The switches are read once per process, so the
cases run in fresh child processes, one after another, each under its own time
limit; the first child that fails or dies ends the run. Each child reports the
route of every call, which proves which kernel ran.

TNN_WGRAD_SPLITS=29 is clamped per shape to ceil(M / 256), so one pinned child
gives z = 1, 1, 4, 29, 1, 1 over the cases below.

Bound against the float64 CPU reference: the one derived in
tests/test_gpu_wgrad_bias.py, |dw - ref| <= 2 * M * 2^-24 * S (S: the reference
on absolute values), likewise db against sum|dy|, plus 2^-7 * |ref| for a bf16
output. It is checked under the default rule and under TNN_WGRAD_WIDE=2 with
the launcher's own z.
"""

import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
EPS = 2.0 ** -24
BF16_ULP = 2.0 ** -7
PIN = "29"

# (N, H, W, Cin, Cout, K, stride, pad)
CASES = {
    # M = 16 < BK; one n-tile; 9 exact row tiles
    "below_bk": (1, 4, 4, 128, 128, 3, 1, 1),
    # M = 192 = 3 chunks: the unrolled loop's skipped second step
    "odd_chunks": (3, 8, 8, 128, 128, 3, 1, 1),
    # Kout = 144: the ragged second row tile
    "ragged_kout": (4, 16, 16, 16, 128, 3, 1, 1),
    # two n-tiles; z = 29 pinned: split boundaries off BK multiples
    "two_ntiles_splits": (32, 16, 16, 256, 256, 3, 1, 1),
    "stride2": (4, 16, 16, 128, 256, 3, 2, 1),
    # 1x1, Kout = 128: exactly one row tile
    "shortcut": (4, 16, 16, 128, 256, 1, 2, 0),
}
IDS = list(CASES)
PINNED_Z = {"below_bk": 1, "odd_chunks": 1, "ragged_kout": 4,
            "two_ntiles_splits": 29, "stride2": 1, "shortcut": 1}

# not eligible for the wide tile: the route they have without this module's
# kernels. (case, dtype, route)
INELIGIBLE = {
    "cout64": ((2, 8, 8, 128, 64, 3, 1, 1), torch.bfloat16, "k_conv_wgrad_tr"),
    "fp32": ((2, 8, 8, 128, 128, 3, 1, 1), torch.float32, "k_conv_wgrad_vec"),
    "nonpow2": ((2, 9, 9, 24, 128, 3, 2, 1), torch.bfloat16, "k_conv_wgrad"),
}

# child name -> environment
CHILDREN = {
    "narrow_pin": {"TNN_WGRAD_WIDE": "0", "TNN_WGRAD_SPLITS": PIN},
    "db_pin": {"TNN_WGRAD_WIDE": "2", "TNN_WGRAD_WIDE_BUF": "1",
               "TNN_WGRAD_SPLITS": PIN},
    "sb_pin": {"TNN_WGRAD_WIDE": "2", "TNN_WGRAD_WIDE_BUF": "2",
               "TNN_WGRAD_SPLITS": PIN},
    "auto": {},
    "wide_free": {"TNN_WGRAD_WIDE": "2"},
}
WIDE_NAME = {"db_pin": "k_conv_wgrad_tr_wide<db>",
             "sb_pin": "k_conv_wgrad_tr_wide<sb>"}
SWITCHES = ("TNN_WGRAD_WIDE", "TNN_WGRAD_WIDE_BUF", "TNN_WGRAD_SPLITS",
            "TNN_WGRAD_WAVES")


def _inputs(case, seed, dtype=torch.bfloat16):
    # CPU generator: every child must see the very same bits
    N, H, W, Ci, Co, K, S, P = case
    g = torch.Generator().manual_seed(seed)
    OH = (H + 2 * P - K) // S + 1
    OW = (W + 2 * P - K) // S + 1
    x = torch.randn(N, H, W, Ci, generator=g).bfloat16().to(dtype)
    dy = torch.randn(N, OH, OW, Co, generator=g).bfloat16().to(dtype)
    return x, dy


def _seed(name):
    return sum(map(ord, name))


def _run_all():
    from tnn_amd import _C
    ext = _C.ext()
    out = {}
    for name, case in CASES.items():
        K, S, P = case[5:]
        x, dy = (t.to(DEV) for t in _inputs(case, _seed(name)))
        args = (x, dy, K, K, S, S, P, P)
        dw, db = ext.conv2d_wgrad_bias(*args, False)
        dw2, db2 = ext.conv2d_wgrad_bias(*args, False)
        dw_bf, db_bf = ext.conv2d_wgrad_bias(*args, True)
        kernel, z = ext.conv2d_wgrad_route(*args)
        out[name] = {
            "kernel": kernel, "z": z,
            "dw": dw.cpu(), "db": db.cpu(),
            "dw_again": dw2.cpu(), "db_again": db2.cpu(),
            "dw_bf": dw_bf.cpu(), "db_bf": db_bf.cpu(),
            "alone": ext.conv2d_wgrad(*args, False).cpu(),
            "alone_bf": ext.conv2d_wgrad(*args, True).cpu(),
        }
    for name, (case, dtype, _) in INELIGIBLE.items():
        K, S, P = case[5:]
        x, dy = (t.to(DEV) for t in _inputs(case, _seed(name), dtype))
        kernel, z = ext.conv2d_wgrad_route(x, dy, K, K, S, S, P, P)
        out[name] = {"kernel": kernel, "z": z}
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def children(tmp_path_factory):
    """Every child's results. Children run one after another; the first that
    fails, dies or runs out of time raises here and none is started after."""
    tmp = tmp_path_factory.mktemp("wgrad_wide")
    out = {}
    for name, switches in CHILDREN.items():
        path = str(tmp / f"{name}.pt")
        env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
        env.update(switches)
        subprocess.run([sys.executable, os.path.abspath(__file__), path],
                       env=env, check=True, timeout=120)
        out[name] = torch.load(path)
    return out


def _route(got):
    return got["kernel"], got["z"]


def _ref_one(x, dy, K, S, P):
    """float64 CPU reference and its absolute-value twin, NHWC-shaped (as in
    tests/test_gpu_wgrad_bias.py)."""
    Ci, Co = x.shape[-1], dy.shape[-1]
    xd = x.double().permute(0, 3, 1, 2)
    dyd = dy.double().permute(0, 3, 1, 2)

    def wg(a, b):
        r = torch.nn.grad.conv2d_weight(a, (Co, Ci, K, K), b, stride=S,
                                        padding=P)
        return r.permute(2, 3, 1, 0)  # -> [KH,KW,Ci,Co]

    return {
        "M": dy.numel() // Co,
        "dw": wg(xd, dyd), "dw_abs": wg(xd.abs(), dyd.abs()),
        "db": dyd.sum(dim=(0, 2, 3)), "db_abs": dyd.abs().sum(dim=(0, 2, 3)),
    }


@pytest.fixture(scope="module")
def refs():
    out = {}
    for name, case in CASES.items():
        x, dy = _inputs(case, _seed(name))
        out[name] = _ref_one(x, dy, *case[5:])
    return out


def _check(dw, db, ref, extra_rel=0.0):
    M = ref["M"]
    for what, got in (("dw", dw), ("db", db)):
        err = (got.double() - ref[what]).abs()
        bound = (2 * M * EPS * ref[what + "_abs"] +
                 extra_rel * ref[what].abs() + 1e-30)
        worst = (err / bound).max().item()
        print(f"{what}: max err/bound {worst:.3g}, "
              f"max err {err.max().item():.3g}")
        assert (err <= bound).all(), f"{what} off: err/bound {worst}"


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["db_pin", "sb_pin"])
@pytest.mark.parametrize("name", IDS)
def test_wide_bitwise_vs_narrow(name, form, children):
    wide, narrow = children[form][name], children["narrow_pin"][name]
    print(name, form, _route(wide), _route(narrow))
    # a run that took the 128x64 kernel twice must not pass
    assert _route(wide) == (WIDE_NAME[form], PINNED_Z[name])
    assert _route(narrow) == ("k_conv_wgrad_tr", PINNED_Z[name])
    for key in ("dw", "db", "dw_bf", "db_bf"):
        assert torch.equal(wide[key], narrow[key]), (name, form, key)


@pytest.mark.gpu
@pytest.mark.parametrize("child", ["auto", "wide_free", "db_pin", "sb_pin"])
@pytest.mark.parametrize("name", IDS)
def test_wide_float64_bound(name, child, children, refs):
    got = children[child][name]
    Ci, Co, K = CASES[name][3:6]
    print(name, child, _route(got))
    if child == "wide_free":
        assert "wide" in got["kernel"], _route(got)
    assert got["dw"].shape == (K, K, Ci, Co)
    assert got["dw"].dtype == torch.float32
    assert got["db"].shape == (Co,) and got["db"].dtype == torch.float32
    _check(got["dw"], got["db"], refs[name])
    assert got["dw_bf"].dtype == torch.bfloat16
    assert got["db_bf"].dtype == torch.bfloat16
    _check(got["dw_bf"], got["db_bf"], refs[name], extra_rel=BF16_ULP)


@pytest.mark.gpu
@pytest.mark.parametrize("child", ["db_pin", "sb_pin", "wide_free", "auto"])
@pytest.mark.parametrize("name", IDS)
def test_wide_alone_and_repeat_bit_identical(name, child, children):
    """conv2d_wgrad agrees with conv2d_wgrad_bias bit for bit (the route does
    not depend on the bias row), and so do two calls."""
    got = children[child][name]
    assert torch.equal(got["alone"], got["dw"]), (name, child)
    assert torch.equal(got["alone_bf"], got["dw_bf"]), (name, child)
    assert torch.equal(got["dw_again"], got["dw"]), (name, child)
    assert torch.equal(got["db_again"], got["db"]), (name, child)


@pytest.mark.gpu
@pytest.mark.parametrize("child", list(CHILDREN))
@pytest.mark.parametrize("name", list(INELIGIBLE))
def test_ineligible_routes_unchanged(name, child, children):
    route = _route(children[child][name])
    print(name, child, route)
    assert route[0] == INELIGIBLE[name][2], (name, child, route)
    assert route[1] >= 1


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    torch.save(_run_all(), sys.argv[1])
