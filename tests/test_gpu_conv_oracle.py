"""Conv fwd / dgrad / wgrad on the GPU against the float64 oracle
(conv_oracle.py).

The route switches are read once per process, so the whole case table runs
in fresh child processes, one per entry of conv_oracle.CHILDREN (default,
TNN_FWD_DB=0, the 128x64 tiles, the 128x128 tiles double-buffered and on one
buffer pair, the last three with the wgrad split count pinned to 29). The
children run one after another, each under its own time limit; the first
that fails, dies or runs out of time raises and none is started after it.
A child runs every case once from guard-banded operands (views into
NaN-filled buffers, an odd element count in for the unaligned cases), calls
every entry point twice, and saves the outputs, whether the second call
returned the same bits, and the route names. The tests then only compare
saved tensors, per case and child:

  the route is the one conv_oracle expects (a case that quietly took
  another kernel must not pass);
  layer 1 equals the exact integer reference bit for bit, statistics and
  both wgrad output types included, and conv2d_wgrad equals
  conv2d_wgrad_bias;
  no output holds a NaN (a read outside an operand that reached an output);
  the second call returned the same bits (layer 2: all but the statistics,
  whose atomics may fold in another order);
  layer 2 stays within the element-wise bound; err / bound is printed.

One case also goes through ops.conv2d_nhwc forward and backward, which
proves that the stride and padding tuples reach the kernels in the right
order. The binding checks at the end raise before any launch.

The 5x5 and 7x7 stride-2 cases run here only because dgrad_parity keeps
them off the parity kernels, whose tap decode handles at most two taps
across; their expected routes are the any-stride ones.
"""

import os
import subprocess
import sys
import time

import pytest
import torch

import conv_oracle as co

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
# about ten times a child's measured wall time on an MI355X (3 to 4 s, most
# of it the interpreter start and the import)
CHILD_TIMEOUT = 40

L1_IDS = [c.id for c in co.cases_for(1)]
L2_IDS = [c.id for c in co.cases_for(2)]
CHILD_NAMES = list(co.CHILDREN)


# ---------------------------------------------------------------------------
# the child: everything that touches the GPU
# ---------------------------------------------------------------------------

def _same_bits(a, b):
    it = torch.int16 if a.dtype == BF16 else torch.int32
    return a.dtype == b.dtype and a.shape == b.shape and \
        torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def _call_all(ext, c, x, w, bias, dy):
    """every entry point of the case once: {key: output}"""
    s = c.conv_args
    out = {}
    if "y" in c.keys:
        out["y"] = ext.conv2d_fwd(x, w, bias, *s, False)
        out["y_relu"] = ext.conv2d_fwd(x, w, bias, *s, True)
        out["y_stats"], out["stats"] = ext.conv2d_fwd_stats(x, w, bias, *s)
    if "dx" in c.keys:
        out["dx"] = ext.conv2d_dgrad(dy, w, c.H, c.W, *s)
    if "dw_f32" in c.keys:
        for tag, out_in_dt in (("f32", False), ("dt", True)):
            args = (x, dy, c.KH, c.KW, *s, out_in_dt)
            out["dw_" + tag] = ext.conv2d_wgrad(*args)
            out["dwb_" + tag], out["db_" + tag] = ext.conv2d_wgrad_bias(*args)
    return out


def _run_case(ext, c, layer):
    x, w, bias, dy = co.device_operands(c, layer, DEV)
    first = _call_all(ext, c, x, w, bias, dy)
    again = _call_all(ext, c, x, w, bias, dy)
    res = {"out": {k: v.cpu() for k, v in first.items()},
           "rep": {k: _same_bits(v, again[k]) for k, v in first.items()}}
    if layer == 1:
        s = c.conv_args
        routes = {"wgrad": tuple(ext.conv2d_wgrad_route(x, dy, c.KH, c.KW,
                                                        *s))}
        if "y" in c.keys:
            routes["fwd"] = ext.conv2d_fwd_route(x, w, *s, False)
            routes["fwd_stats"] = ext.conv2d_fwd_route(x, w, *s, True)
        if "dx" in c.keys:
            routes["dgrad"] = ext.conv2d_dgrad_route(dy, w, c.H, c.W, *s)
        res["routes"] = routes
        if c.nhwc:
            res["nhwc"] = _run_nhwc(c, x, w, bias, dy)
    return res


def _run_nhwc(c, x, w, bias, dy):
    from tnn_amd import ops
    x, w, bias = (t.detach().requires_grad_() for t in (x, w, bias))
    y = ops.conv2d_nhwc(x, w, bias, stride=(c.SH, c.SW),
                        padding=(c.PH, c.PW))
    y.backward(dy)
    return {"nhwc_y": y.detach().cpu(), "nhwc_dx": x.grad.cpu(),
            "nhwc_dw": w.grad.cpu(), "nhwc_db": bias.grad.cpu()}


def _run_all():
    from tnn_amd import _C
    ext = _C.ext()
    out = {1: {}, 2: {}}
    for layer in (1, 2):
        for c in co.cases_for(layer):
            out[layer][c.id] = _run_case(ext, c, layer)
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def children(tmp_path_factory):
    """Every child's results. Children run one after another; the first that
    fails, dies or runs out of time raises here and none is started after."""
    tmp = tmp_path_factory.mktemp("conv_oracle")
    out = {}
    for name, switches in co.CHILDREN.items():
        path = str(tmp / f"{name}.pt")
        env = {k: v for k, v in os.environ.items() if k not in co.SWITCHES}
        env.update(switches)
        t0 = time.time()
        subprocess.run([sys.executable, os.path.abspath(__file__), path],
                       env=env, check=True, timeout=CHILD_TIMEOUT)
        print(f"child {name}: {time.time() - t0:.1f} s")
        out[name] = torch.load(path)
    return out


# ---------------------------------------------------------------------------
# the tests: saved tensors against the oracle
# ---------------------------------------------------------------------------

def _got(children, child, layer, cid):
    return children[child][layer][cid]


@pytest.mark.parametrize("child", CHILD_NAMES)
@pytest.mark.parametrize("cid", L1_IDS)
def test_route_is_the_expected_one(cid, child, children):
    c = co.BY_ID[cid]
    got = _got(children, child, 1, cid)["routes"]
    want = co.expected_routes(c, child)
    print(cid, child, got)
    for k, v in got.items():
        assert v == want[k], (cid, child, k, v, want[k])


@pytest.mark.parametrize("child", CHILD_NAMES)
@pytest.mark.parametrize("cid", L1_IDS)
def test_layer1_equals_the_exact_reference(cid, child, children):
    c = co.BY_ID[cid]
    res = _got(children, child, 1, cid)
    out = res["out"]
    assert set(out) == set(c.keys)
    has_stats = co.fwd_dma(c, child)
    diffs = {}
    for key in c.keys:
        if key == "stats" and not has_stats:
            # the register-staged routes carry no statistics epilogue
            assert out[key].numel() == 0, (cid, child)
            continue
        diffs[key] = co.check_exact(out[key], c, key)
    print(f"{cid} {child}: " + "  ".join(f"{k} {d:g}"
                                         for k, d in diffs.items()))
    for key, d in diffs.items():
        assert d == 0.0, f"{cid} {child} {key}: differs from the exact " \
                         f"reference by up to {d}"
    for a, b in co.SAME_DW:
        if a in out:
            assert torch.equal(out[a], out[b]), (cid, child, a, b)
    for key, ref_key in co.NHWC_KEYS.items():
        if c.nhwc:
            assert co.check_exact(res["nhwc"][key], c, ref_key) == 0.0, \
                (cid, child, key)


@pytest.mark.parametrize("child", CHILD_NAMES)
@pytest.mark.parametrize("layer,cid", [(1, i) for i in L1_IDS]
                         + [(2, i) for i in L2_IDS])
def test_no_nan_and_second_call_bit_identical(layer, cid, child, children):
    res = _got(children, child, layer, cid)
    for key, t in res["out"].items():
        assert not torch.isnan(t).any(), (cid, child, key)
        # layer 2: the statistics' atomics may fold in another order
        if not (layer == 2 and key == "stats"):
            assert res["rep"][key], f"{cid} {child} {key}: second call " \
                                    f"returned other bits"
    for t in res.get("nhwc", {}).values():
        assert not torch.isnan(t).any(), (cid, child)


@pytest.mark.parametrize("child", CHILD_NAMES)
@pytest.mark.parametrize("cid", L2_IDS)
def test_layer2_within_the_bound(cid, child, children):
    c = co.BY_ID[cid]
    out = _got(children, child, 2, cid)["out"]
    has_stats = co.fwd_dma(c, child)
    ratios = {}
    for key in c.keys:
        if key == "stats" and not has_stats:
            assert out[key].numel() == 0, (cid, child)
            continue
        ratios[key] = co.check_bound(out[key], c, key)
    print(f"{cid} {child}: err / bound " +
          "  ".join(f"{k} {r:.3f}" for k, r in ratios.items()))
    for key, r in ratios.items():
        assert r <= 1.0, f"{cid} {child} {key}: {r:.3f} bounds from float64"
    for a, b in co.SAME_DW:
        assert torch.equal(out[a], out[b]), (cid, child, a, b)


# ---------------------------------------------------------------------------
# binding checks: all of these raise before any launch
# ---------------------------------------------------------------------------

class _Ext:
    """the extension, imported at the first call (a child process runs this
    file as a script, before the package is on its path)"""

    def __getattr__(self, name):
        from tnn_amd import _C
        return getattr(_C.ext(), name)


ext = _Ext()


def _t(*shape, dtype=BF16, device=DEV):
    return torch.ones(*shape, dtype=dtype, device=device)


def _fwd_calls(x, w, bias, s):
    return [lambda: ext.conv2d_fwd(x, w, bias, *s, False),
            lambda: ext.conv2d_fwd_stats(x, w, bias, *s)]


def _all_calls(x, w, dy, H, W, KH, KW, s, bias=None):
    return _fwd_calls(x, w, bias, s) + [
        lambda: ext.conv2d_fwd_route(x, w, *s, False),
        lambda: ext.conv2d_dgrad(dy, w, H, W, *s),
        lambda: ext.conv2d_dgrad_route(dy, w, H, W, *s),
        lambda: ext.conv2d_wgrad(x, dy, KH, KW, *s, False),
        lambda: ext.conv2d_wgrad_bias(x, dy, KH, KW, *s, False),
        lambda: ext.conv2d_wgrad_route(x, dy, KH, KW, *s)]


def test_fwd_rejects_a_bad_bias():
    x, w, s = _t(1, 8, 8, 16), _t(3, 3, 16, 32), (1, 1, 1, 1)
    for bad in (_t(31), _t(33), _t(64)[::2], _t(32, device="cpu")):
        for f in _fwd_calls(x, w, bad, s):
            with pytest.raises(RuntimeError, match="bias must be a contiguous "
                                                   "GPU tensor of 32"):
                f()
    for f in _fwd_calls(x, w, _t(32, dtype=F32), s):
        with pytest.raises(RuntimeError, match="bias dtype mismatch"):
            f()


@pytest.mark.parametrize("s,msg", [((0, 1, 1, 1), "stride must be >= 1"),
                                   ((1, 0, 1, 1), "stride must be >= 1"),
                                   ((1, -1, 1, 1), "stride must be >= 1"),
                                   ((1, 1, -1, 1), "padding must be >= 0"),
                                   ((1, 1, 1, -1), "padding must be >= 0")])
def test_every_entry_point_rejects_bad_strides_and_pads(s, msg):
    x, w, dy = _t(1, 8, 8, 16), _t(3, 3, 16, 16), _t(1, 8, 8, 16)
    for f in _all_calls(x, w, dy, 8, 8, 3, 3, s):
        with pytest.raises(RuntimeError, match=msg):
            f()


def test_every_entry_point_rejects_an_input_smaller_than_the_kernel():
    # 2 x 8 input, 3 x 3 kernel, no padding: (2 - 3) / 2 + 1 rounds to 1 in C
    x, w, dy = _t(1, 2, 8, 16), _t(3, 3, 16, 16), _t(1, 1, 3, 16)
    for f in _all_calls(x, w, dy, 2, 8, 3, 3, (2, 2, 0, 0)):
        with pytest.raises(RuntimeError, match="no output pixel"):
            f()


@pytest.mark.parametrize("dim", ["N", "H", "Cin", "Cout", "KH"])
def test_every_entry_point_rejects_an_empty_dimension(dim):
    d = {k: (0 if k == dim else v) for k, v in
         dict(N=1, H=8, Cin=16, Cout=16, KH=3).items()}
    x = _t(d["N"], d["H"], 8, d["Cin"])
    w = _t(d["KH"], 3, d["Cin"], d["Cout"])
    dy = _t(d["N"], d["H"], 8, d["Cout"])
    for f in _all_calls(x, w, dy, d["H"], 8, d["KH"], 3, (1, 1, 1, 1)):
        with pytest.raises(RuntimeError, match="empty operand|no output pixel"):
            f()


def test_dgrad_rejects_operands_it_used_to_trust():
    w, s = _t(3, 3, 16, 32), (1, 1, 1, 1)
    cases = [
        (_t(8, 8, 32), 8, 8, r"conv2d_dgrad\w* dy"),                # 3-d
        (_t(1, 8, 8, 32, dtype=F32), 8, 8, "dtype mismatch: dy is"),
        (_t(1, 8, 8, 16), 8, 8, "other channels than w"),
        (_t(1, 7, 8, 32), 8, 8, "is not the output of a 8 x 8 input"),
        (_t(1, 8, 8, 32), 8, 16, "is not the output of a 8 x 16 input"),
        (_t(0, 8, 8, 32), 8, 8, "empty operand"),
    ]
    for dy, H, W, msg in cases:
        for f in (lambda: ext.conv2d_dgrad(dy, w, H, W, *s),
                  lambda: ext.conv2d_dgrad_route(dy, w, H, W, *s)):
            with pytest.raises(RuntimeError, match=msg):
                f()
    with pytest.raises(RuntimeError, match=r"conv2d_dgrad dy"):
        ext.conv2d_dgrad(_t(1, 8, 8, 32), _t(3, 16, 32), 8, 8, *s)


def test_wgrad_rejects_operands_it_used_to_trust():
    s = (1, 1, 1, 1)
    cases = [
        (_t(8, 8, 16), _t(1, 8, 8, 32), r"conv2d_wgrad\w* x"),       # 3-d
        (_t(1, 8, 8, 16), _t(8, 8, 32), r"conv2d_wgrad\w* x"),
        (_t(1, 8, 8, 16, dtype=F32), _t(1, 8, 8, 32),
         "dtype mismatch: x is"),
        (_t(2, 8, 8, 16), _t(1, 8, 8, 32), "batch mismatch"),
        (_t(1, 8, 8, 16), _t(1, 7, 8, 32), "wgrad shape"),
    ]
    for x, dy, msg in cases:
        for f in (lambda: ext.conv2d_wgrad(x, dy, 3, 3, *s, False),
                  lambda: ext.conv2d_wgrad_bias(x, dy, 3, 3, *s, True),
                  lambda: ext.conv2d_wgrad_route(x, dy, 3, 3, *s)):
            with pytest.raises(RuntimeError, match=msg):
                f()


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    torch.save(_run_all(), sys.argv[1])
