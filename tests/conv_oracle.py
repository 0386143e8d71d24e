"""Oracle for the convolution kernels (conv2d.hip): case table, inputs,
float64 references, conditions, bounds, expected routes and wrong variants,
shared by test_conv_oracle_cpu.py and test_gpu_conv_oracle.py. The conv
counterpart of gemm_oracle.py, whose pieces it reuses (guarded, bf16_spacing,
U, ACC_FLOOR, ACC_FACTOR, TEETH).

Everything here is torch on the CPU and nothing imports the extension.

Canonical form. Every direction is a GEMM out[P, Q] = sum_r A[p, r] B[r, q]
over a gathered operand, built here from index arithmetic (not from
F.conv2d, which the CPU test uses as the independent honest model):

  fwd    A = im2col(x) [M, K],   B = w [K, Cout]          R = K = KH KW Cin
  dgrad  A = gathered dy [N H W, KH KW Cout], B = w^T     R = KH KW Cout
  wgrad  A = im2col(x)^T [K, M], B = dy [M, Cout]         R = M = N OH OW
  db     column sums of dy                                R = M

A case runs every entry point: conv2d_fwd linear and relu, conv2d_fwd_stats,
conv2d_dgrad, conv2d_wgrad and conv2d_wgrad_bias with fp32 and same-dtype
output. KEYS names the outputs. Operands are contiguous views into
NaN-filled buffers (gemm_oracle.guarded), 16-byte aligned or, in the cases
marked unaligned, an odd element count in, where the vector gate fails and
the <pow2> / generic kernels must return the same exact result.

Layer 1, exact. x, w, dy hold +-1 and +-2, bias integers. With S the same
computation on absolute values, S < 2^24 (exact_conditions asserts it), so
every partial sum in any order is an integer below 2^24, exact in fp32, and
each output must equal ref64.to(dtype) bit for bit. The fused statistics
need sum_m |y| < 2^24 and sum_m y^2 < 2^24 per channel and must then equal
the float64 sums of the unrounded y, as fp32. Measured on the CPU over the
table: S <= 17030, sum |y| <= 26192, sum y^2 <= 3.84e6.

Layer 2, precision. x = randn, w = 0.1 randn, bias = 0.5 randn, dy = randn,
rounded to the dtype; float64 reference from the rounded inputs. Bound per
element, with u = 2^-24 and S the absolute-value twin of the pre-activation:

  min(ACC_FACTOR ACC_FLOOR sqrt(R), 2 R) u S + 2 u |ref| + 1e-30

and half the bf16 spacing at `got` taken off the error of a bf16 output
(gemm_oracle's output-rounding argument). The activation is linear or relu:
slope at most 1, no evaluation error. Statistics: against the float64 sums
of the float64 y; with d_m the bound of element m, the column sum may be off
by sum_m d_m + min(ACC sqrt(M), 2 M) u sum_m |y|, the sum of squares by
sum_m (2 |y| d_m + d_m^2) + min(ACC sqrt(M), 2 M) u sum_m y^2 (+ one more
u sum y^2 for the squares' own rounding). ACC_FLOOR = 0.7 and ACC_FACTOR = 4
are gemm_oracle's: the honest fp32 model (fp32 F.conv2d and torch.nn.grad,
one output rounding) reaches err / (sqrt(R) u S) = 0.635 on these cases
(CPU, re-measured by the CPU test, which asserts it stays below the floor),
so the conv summation shapes need no larger floor.

Wrong variants. Layer 1 (VARIANTS1): each is unequal on every (case, output)
it applies to. Layer 2 (VARIANTS2): each lands at least TEETH = 3 bounds
away wherever it applies; smallest distances measured by the CPU test
(MEASURED_TEETH):

  slab_bf16 45.58   acc_bf16 157.47   stats_rounded 7.38

slab_bf16 applies to y, dx, dw and db of every layer-2 case, acc_bf16 to
every fp32 output, stats_rounded (statistics from the bf16-rounded y) to the
statistics of every bf16 case; no case had to be excused from a variant.
Against the plain bound 2 R u S + 2^-7 |ref| the same three land as near as
1.42, 9.25 and 0.31.
"""

import functools

import torch
import torch.nn.functional as F

from gemm_oracle import (ACC_FACTOR, ACC_FLOOR, BF16, BF16_ULP, F32, GUARD,
                         TEETH, U, bf, bf16_spacing, dt_name, guarded,
                         hash_str)

# GUARD and TEETH are here for the two test modules

# smallest measured distance per layer-2 variant (CPU, this module's cases)
MEASURED_TEETH = {"slab_bf16": 45.58, "acc_bf16": 157.47,
                  "stats_rounded": 7.38}

ACC = ACC_FACTOR * ACC_FLOOR

# output key -> (direction, output dtype: "dt" the case's, "f32")
KEYS = {
    "y": ("fwd", "dt"), "y_relu": ("fwd", "dt"), "y_stats": ("fwd", "dt"),
    "stats": ("fwd", "f32"),
    "dx": ("dgrad", "dt"),
    "dw_f32": ("wgrad", "f32"), "dw_dt": ("wgrad", "dt"),
    "dwb_f32": ("wgrad", "f32"), "dwb_dt": ("wgrad", "dt"),
    "db_f32": ("db", "f32"), "db_dt": ("db", "dt"),
}
# conv2d_wgrad and conv2d_wgrad_bias must agree bit for bit
SAME_DW = (("dw_f32", "dwb_f32"), ("dw_dt", "dwb_dt"))
# ops.conv2d_nhwc forward / backward outputs -> the key they must equal
NHWC_KEYS = {"nhwc_y": "y", "nhwc_dx": "dx", "nhwc_dw": "dw_dt",
             "nhwc_db": "db_dt"}


def _pow2(v):
    return v >= 1 and (v & (v - 1)) == 0


def _cdiv(a, b):
    return -(-a // b)


class Case:
    """(N, H, W, Cin, Cout, KH, KW, SH, SW, PH, PW, dtype) under a label"""

    def __init__(self, label, N, H, W, Cin, Cout, KH, KW, SH, SW, PH, PW,
                 dtype=BF16, *, layers=(1,), unaligned=False, nhwc=False,
                 only=None):
        self.label, self.dtype = label, dtype
        self.N, self.H, self.W, self.Cin, self.Cout = N, H, W, Cin, Cout
        self.KH, self.KW, self.SH, self.SW = KH, KW, SH, SW
        self.PH, self.PW = PH, PW
        self.layers, self.unaligned, self.nhwc = tuple(layers), unaligned, nhwc
        self.OH = (H + 2 * PH - KH) // SH + 1
        self.OW = (W + 2 * PW - KW) // SW + 1
        assert self.OH >= 1 and self.OW >= 1
        self.T = KH * KW
        self.M = N * self.OH * self.OW          # fwd rows, wgrad reduction
        self.K = self.T * Cin                   # fwd reduction
        self.Rd = self.T * Cout                 # dgrad reduction
        self.keys = tuple(k for k in KEYS
                          if only is None or KEYS[k][0] in only)

    @property
    def conv_args(self):
        return (self.SH, self.SW, self.PH, self.PW)

    @property
    def id(self):
        s = (f"{self.label}-{dt_name(self.dtype)}-{self.N}x{self.H}x{self.W}"
             f"x{self.Cin}x{self.Cout}-k{self.KH}x{self.KW}"
             f"-s{self.SH}x{self.SW}-p{self.PH}x{self.PW}")
        return s + ("-unal" if self.unaligned else "")

    def __repr__(self):
        return self.id

    @property
    def seed(self):
        return (hash_str(self.id) % (2 ** 31 - 1)) + 1

    def R(self, key):
        return {"fwd": self.K, "dgrad": self.Rd, "wgrad": self.M,
                "db": self.M}[KEYS[key][0]]

    def out_dtype(self, key):
        return F32 if KEYS[key][1] == "f32" else self.dtype


def _cases():
    C = Case
    sq = lambda k, s, p: (k, k, s, s, p, p)
    out = [
        # what test_gpu_conv_db / _conv_wide / _wgrad_wide enumerate
        C("chunk1_mtail", 1, 8, 8, 64, 128, *sq(1, 1, 0)),
        C("chunk2", 1, 8, 8, 128, 128, *sq(1, 1, 0)),
        C("chunk9_odd", 1, 8, 8, 64, 128, *sq(3, 1, 1), layers=(1, 2)),
        C("m128_k1152", 2, 8, 8, 128, 128, *sq(3, 1, 1), layers=(1, 2)),
        C("ragged_k144", 1, 8, 8, 16, 128, *sq(3, 1, 1), layers=(1, 2)),
        C("slices_cin32", 1, 8, 8, 32, 64, *sq(3, 1, 1)),
        C("tails_cout16", 1, 4, 4, 128, 16, *sq(3, 1, 1)),
        C("tiles_fwd", 4, 8, 8, 128, 256, *sq(3, 1, 1)),
        C("tiles_dgrad_k2304", 4, 8, 8, 256, 128, *sq(3, 1, 1)),
        C("s2_parity", 4, 8, 8, 128, 256, *sq(3, 2, 1), layers=(1, 2)),
        C("s2_1x1_tapless", 2, 8, 8, 128, 256, *sq(1, 2, 0)),
        C("k4608", 1, 4, 4, 512, 512, *sq(3, 1, 1)),
        C("stride4", 1, 16, 16, 128, 128, *sq(3, 4, 1)),
        C("wgrad_below_bk", 1, 4, 4, 128, 128, *sq(3, 1, 1)),
        C("wgrad_3chunks", 3, 8, 8, 128, 128, *sq(3, 1, 1)),
        C("wgrad_kout144", 4, 16, 16, 16, 128, *sq(3, 1, 1)),
        # M = 7424 = 29 * 256: the pinned split count z = 29 is not clamped
        C("wgrad_z29", 29, 16, 16, 32, 256, *sq(3, 1, 1),
          only=("wgrad", "db")),
        # H != W, narrow and wide tile in every direction
        C("rect_8x16", 2, 8, 16, 64, 128, *sq(3, 1, 1), layers=(1, 2)),
        C("rect_16x4", 2, 16, 4, 128, 64, *sq(3, 1, 1)),
        C("rect_s2_8x16", 2, 8, 16, 128, 128, *sq(3, 2, 1)),
        C("rect_1x1", 2, 8, 16, 64, 64, *sq(1, 1, 0)),
        # KH != KW (and with it PH != PW on the all-pow2 routes)
        C("k3x1", 2, 8, 8, 64, 64, 3, 1, 1, 1, 1, 0),
        C("k1x3", 2, 8, 8, 64, 64, 1, 3, 1, 1, 0, 1),
        # parity route with nkh = 3, nkw <= 2 and start_h != start_w
        C("k5x3_s2_p2x1", 2, 8, 16, 64, 128, 5, 3, 2, 2, 2, 1,
          layers=(1, 2)),
        # KW = 4: the widest kernel the parity route takes
        C("k4x4_s2", 2, 8, 8, 64, 64, *sq(4, 2, 1)),
        # SH != SW: any-stride dgrad, plain forward
        C("s2x1", 2, 8, 8, 64, 64, 3, 3, 2, 1, 1, 1, layers=(1, 2)),
        C("s1x2", 2, 8, 8, 128, 128, 3, 3, 1, 2, 1, 1),
        # PH != PW with 3x3 (one output extent is then no power of two)
        C("p1x0", 2, 8, 8, 64, 64, 3, 3, 1, 1, 1, 0),
        C("p0x1", 2, 8, 8, 64, 64, 3, 3, 1, 1, 0, 1),
        # no tap in the padding, the output shrinks
        C("pad0_3x3", 2, 8, 8, 64, 64, *sq(3, 1, 0)),
        # stride 2 with more than 2 taps across: off the parity route
        C("k5x5_s2", 2, 8, 8, 16, 16, *sq(5, 2, 2)),
        C("k7x7_s2", 2, 8, 8, 16, 16, *sq(7, 2, 3)),
        C("k5x5_s2_wide", 2, 8, 8, 128, 128, *sq(5, 2, 2)),
        C("k7x7_s2_wide", 2, 8, 8, 128, 128, *sq(7, 2, 3)),
        # magic-number division and the generic kernels
        C("nonpow2", 2, 9, 7, 24, 40, 3, 3, 2, 1, 1, 1, layers=(1, 2)),
        C("nonpow2", 2, 9, 7, 24, 40, 3, 3, 2, 1, 1, 1, F32, layers=(1, 2)),
        # fp32 on every route it has
        C("f32_db", 1, 8, 8, 64, 64, *sq(3, 1, 1), F32, layers=(1, 2)),
        C("f32_db_k2304", 1, 4, 4, 256, 64, *sq(3, 1, 1), F32),
        C("f32_glds_k4608", 1, 4, 4, 512, 64, *sq(3, 1, 1), F32),
        C("f32_s2_parity", 2, 8, 8, 64, 64, *sq(3, 2, 1), F32,
          layers=(1, 2)),
        C("f32_rect_k3x1", 2, 8, 16, 32, 64, 3, 1, 1, 1, 1, 0, F32),
        # operands an odd element count into their buffers
        C("chunk9_odd", 1, 8, 8, 64, 128, *sq(3, 1, 1), unaligned=True),
        C("f32_db", 1, 8, 8, 64, 64, *sq(3, 1, 1), F32, unaligned=True),
        C("s2_parity", 2, 8, 8, 64, 128, *sq(3, 2, 1), unaligned=True),
        # everything unequal at once, also through ops.conv2d_nhwc
        C("nhwc_rect_s2x1", 2, 8, 16, 64, 64, 3, 1, 2, 1, 1, 0,
          layers=(1, 2), nhwc=True),
    ]
    return out


CASES = _cases()
assert len({c.id for c in CASES}) == len(CASES)
BY_ID = {c.id: c for c in CASES}


def cases_for(layer):
    return [c for c in CASES if layer in c.layers]


# ---------------------------------------------------------------------------
# expected routes: the dispatch rules of docs/KERNELS.md ("Conv routes"),
# written down once more from the document
# ---------------------------------------------------------------------------

CHILDREN = {
    "default": {},
    "nodb": {"TNN_FWD_DB": "0"},
    "narrow": {"TNN_CONV_WIDE": "0", "TNN_WGRAD_WIDE": "0",
               "TNN_WGRAD_SPLITS": "29"},
    "wide_db": {"TNN_CONV_WIDE": "2", "TNN_CONV_WIDE_BUF": "1",
                "TNN_WGRAD_WIDE": "2", "TNN_WGRAD_WIDE_BUF": "1",
                "TNN_WGRAD_SPLITS": "29"},
    "wide_sb": {"TNN_CONV_WIDE": "2", "TNN_CONV_WIDE_BUF": "2",
                "TNN_WGRAD_WIDE": "2", "TNN_WGRAD_WIDE_BUF": "2",
                "TNN_WGRAD_SPLITS": "29"},
}
# every conv switch; a child's environment holds only those of its entry
SWITCHES = ("TNN_FWD_DB", "TNN_DB_MAXK", "TNN_DB_MAXK_DGRAD",
            "TNN_CONV_WIDE", "TNN_CONV_WIDE_BUF", "TNN_WGRAD_WIDE",
            "TNN_WGRAD_WIDE_BUF", "TNN_WGRAD_SPLITS", "TNN_WGRAD_WAVES")

# every name the three conv2d_*_route functions can return
FWD_ROUTES = ("k_conv_fwd_sb_wide", "k_conv_fwd_db_wide", "k_conv_fwd_sb",
              "k_conv_fwd_db", "k_conv_fwd<pow2, glds>", "k_conv_fwd<pow2>",
              "k_conv_fwd")
DGRAD_ROUTES = tuple(
    [f"k_conv_dgrad_{b}{s}" for b in ("sb_wide", "db_wide", "db")
     for s in ("<S2>", "<S1>", "")]
    + ["k_conv_dgrad<pow2, glds, S2>", "k_conv_dgrad<pow2, glds, S1>",
       "k_conv_dgrad<pow2, glds>", "k_conv_dgrad<pow2>", "k_conv_dgrad"])
WGRAD_ROUTES = ("k_conv_wgrad_tr_wide<db>", "k_conv_wgrad_tr_wide<sb>",
                "k_conv_wgrad_tr", "k_conv_wgrad_vec", "k_conv_wgrad<pow2>",
                "k_conv_wgrad")
DB_MAXK, DB_MAXK_DGRAD = 2304, 4608


def _env(child, name, dflt):
    return int(CHILDREN[child].get(name, dflt))


def _all_pow2(c):
    return all(_pow2(v) for v in (c.OH * c.OW, c.OW, c.Cin, c.H * c.W, c.W,
                                  c.Cout))


def _vec(c, channels):
    return channels % (8 if c.dtype == BF16 else 4) == 0 and not c.unaligned


def _wide_pick(mode, buf, eligible, tiles, take, single):
    """None, "db" or "sb" (the table under "wide" in docs/KERNELS.md)"""
    if not eligible or mode == 0:
        return None
    if mode == 1 and not (take and tiles >= 512):
        return None
    if buf:
        single = buf == 2
    return "sb" if single else "db"


def fwd_dma(c, child):
    """the DMA-staged forward routes, which also carry the statistics"""
    return (_env(child, "TNN_FWD_DB", 1) != 0
            and not (c.dtype == F32 and c.K > DB_MAXK)
            and _all_pow2(c) and _vec(c, c.Cin))


def fwd_route(c, child, stats=False):
    if fwd_dma(c, child):
        nt = c.Cout // 128
        wide = _wide_pick(
            _env(child, "TNN_CONV_WIDE", 1),
            _env(child, "TNN_CONV_WIDE_BUF", 0),
            c.dtype == BF16 and c.Cout % 128 == 0, _cdiv(c.M, 128) * nt,
            (not stats) if nt == 1 else c.K >= 2048, nt == 1)
        if wide:
            return f"k_conv_fwd_{wide}_wide"
        long_k = c.dtype == BF16 and c.K > DB_MAXK
        return "k_conv_fwd_sb" if long_k else "k_conv_fwd_db"
    if not _all_pow2(c):
        return "k_conv_fwd"
    return "k_conv_fwd<pow2, glds>" if _vec(c, c.Cin) else "k_conv_fwd<pow2>"


def dgrad_parity(c):
    """parity = all-pow2, stride 2x2, even H and W, KW <= 4, pow2 per-class
    divisors"""
    return (_all_pow2(c) and c.SH == 2 and c.SW == 2 and c.H % 2 == 0
            and c.W % 2 == 0 and c.KW <= 4
            and _pow2((c.H // 2) * (c.W // 2)) and _pow2(c.W // 2))


def dgrad_route(c, child):
    s2 = dgrad_parity(c)
    s1 = c.SH == 1 and c.SW == 1
    form = "S2" if s2 else ("S1" if s1 else "")
    p2, vec = _all_pow2(c), _vec(c, c.Cout)
    if (_env(child, "TNN_FWD_DB", 1) != 0 and c.Rd <= DB_MAXK_DGRAD and p2
            and vec):
        Mc = c.N * (c.H // 2) * (c.W // 2) if s2 else c.N * c.H * c.W
        taps = _cdiv(c.KH, 2) * _cdiv(c.KW, 2) if s2 else c.T
        wide = _wide_pick(
            _env(child, "TNN_CONV_WIDE", 1),
            _env(child, "TNN_CONV_WIDE_BUF", 0),
            c.dtype == BF16 and c.Cin % 128 == 0,
            _cdiv(Mc, 128) * (c.Cin // 128) * (4 if s2 else 1), True,
            taps * c.Cout <= 1152)
        name = f"k_conv_dgrad_{wide}_wide" if wide else "k_conv_dgrad_db"
        return name + (f"<{form}>" if form else "")
    if p2 and vec:
        return "k_conv_dgrad<pow2, glds" + (f", {form}>" if form else ">")
    return "k_conv_dgrad<pow2>" if p2 else "k_conv_dgrad"


def wgrad_route(c, child):
    """(kernel name, split-M count z)"""
    cap = max(_cdiv(c.M, 256), 1)
    pin = _env(child, "TNN_WGRAD_SPLITS", 0)
    name, wide = None, None
    if _all_pow2(c) and _vec(c, c.Cin) and _vec(c, c.Cout):
        if c.dtype == F32:
            name = "k_conv_wgrad_vec"
        else:
            mode = _env(child, "TNN_WGRAD_WIDE", 1)
            buf = _env(child, "TNN_WGRAD_WIDE_BUF", 0)
            nt = c.Cout // 128
            tiles = _cdiv(c.K, 128) * nt
            if c.Cout % 128 == 0 and mode != 0:
                if nt == 1 and c.K > 144:
                    auto = None
                elif cap < 512 // tiles:
                    auto = None
                else:
                    auto = "sb" if tiles >= 144 else "db"
                if mode == 2 or auto:
                    wide = {1: "db", 2: "sb"}.get(buf, auto or "db")
            name = f"k_conv_wgrad_tr_wide<{wide}>" if wide else \
                "k_conv_wgrad_tr"
    else:
        name = "k_conv_wgrad<pow2>" if _all_pow2(c) else "k_conv_wgrad"
    if pin > 0:
        return name, min(pin, cap)
    if wide:
        slots = 512 if wide == "db" else 768
        return name, max(min(cap, slots // (_cdiv(c.K, 128) * (c.Cout // 128))),
                         1)
    base = _cdiv(c.K, 128) * _cdiv(c.Cout, 64)
    return name, max(1 if base >= 2048 else min(cap, _cdiv(2048, base)), 1)


def expected_routes(c, child):
    return {"fwd": fwd_route(c, child), "fwd_stats": fwd_route(c, child, True),
            "dgrad": dgrad_route(c, child), "wgrad": wgrad_route(c, child),
            "has_stats": fwd_dma(c, child)}


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------

def _ints(shape, mags, g):
    m = torch.tensor(mags)[torch.randint(0, len(mags), shape, generator=g)]
    sign = torch.randint(0, 2, shape, generator=g, dtype=torch.int64) * 2 - 1
    return (sign * m).double()


class Inputs:
    """x [N,H,W,Cin], w [KH,KW,Cin,Cout], bias [Cout], dy [N,OH,OW,Cout] as
    float64 holding integers (layer 1) or dtype values (layer 2)"""

    def __init__(self, c, layer):
        g = torch.Generator().manual_seed(c.seed + layer)
        xs = (c.N, c.H, c.W, c.Cin)
        ws = (c.KH, c.KW, c.Cin, c.Cout)
        ys = (c.N, c.OH, c.OW, c.Cout)
        if layer == 1:
            self.x, self.w = _ints(xs, (1, 2), g), _ints(ws, (1, 2), g)
            self.bias = _ints((c.Cout,), (1, 2, 3, 5, 8), g)
            self.dy = _ints(ys, (1, 2), g)
        else:
            rd = lambda t: t.to(c.dtype).double()
            self.x = rd(torch.randn(xs, generator=g))
            self.w = rd(0.1 * torch.randn(ws, generator=g))
            self.bias = rd(0.5 * torch.randn(c.Cout, generator=g))
            self.dy = rd(torch.randn(ys, generator=g))

    def abs(self):
        a = object.__new__(Inputs)
        a.x, a.w, a.bias, a.dy = (self.x.abs(), self.w.abs(), self.bias.abs(),
                                  self.dy.abs())
        return a


@functools.lru_cache(maxsize=None)
def inputs(c, layer):
    return Inputs(c, layer)


def device_operands(c, layer, device):
    """guard-banded (x, w, bias, dy) of the case's dtype on `device`"""
    inp = inputs(c, layer)
    return tuple(guarded(t, c.dtype, device, c.unaligned)
                 for t in (inp.x, inp.w, inp.bias, inp.dy))


# ---------------------------------------------------------------------------
# the gathered operands, with the wrong decodes
# ---------------------------------------------------------------------------

def _taps(c, swap_k):
    kidx = torch.arange(c.T)
    div = c.KH if swap_k else c.KW
    return kidx // div, kidx % div


def fwd_gather(c, x, *, swap_hw=False, swap_p=False, swap_s=False,
               swap_k=False, wrap=False):
    """im2col(x) [M, T * Cin]: row (n, oh, ow), column (kh, kw, ci)"""
    SH, SW = (c.SW, c.SH) if swap_s else (c.SH, c.SW)
    PH, PW = (c.PW, c.PH) if swap_p else (c.PH, c.PW)
    gm = torch.arange(c.M)
    n, rem = gm // (c.OH * c.OW), gm % (c.OH * c.OW)
    ow_div = c.OH if swap_hw else c.OW
    oh, ow = rem // ow_div, rem % ow_div
    kh, kw = _taps(c, swap_k)
    ih = oh[:, None] * SH - PH + kh[None]
    iw = ow[:, None] * SW - PW + kw[None]
    pix = (n[:, None] * c.H + ih) * c.W + iw
    npix = c.N * c.H * c.W
    if wrap:      # the flat address is used wherever it is inside the tensor
        valid = (pix >= 0) & (pix < npix)
    else:
        valid = (ih >= 0) & (ih < c.H) & (iw >= 0) & (iw < c.W)
    A = x.reshape(npix, c.Cin)[pix.clamp(0, npix - 1)]
    return (A * valid[..., None]).reshape(c.M, c.T * c.Cin)


def _last_short_tap(c):
    """the tap through which dy's last row reaches dx's last row, or None"""
    kh = c.H - 1 + c.PH - (c.OH - 1) * c.SH
    return kh if 0 <= kh < c.KH else None


def dgrad_gather(c, dy, *, swap_hw=False, swap_p=False, swap_s=False,
                 swap_k=False, start_nopad=False, last_short=False):
    """gathered dy [N H W, T * Cout]: row (n, ih, iw), column (kh, kw, co)"""
    SH, SW = (c.SW, c.SH) if swap_s else (c.SH, c.SW)
    PH, PW = (c.PW, c.PH) if swap_p else (c.PH, c.PW)
    gm = torch.arange(c.N * c.H * c.W)
    n, rem = gm // (c.H * c.W), gm % (c.H * c.W)
    w_div = c.H if swap_hw else c.W
    ih, iw = rem // w_div, rem % w_div
    kh, kw = _taps(c, swap_k)

    def axis(i, k, P, S, O):
        t = i[:, None] + P - k[None]
        if start_nopad:
            # stride 2: the class takes the taps of its own parity, as if
            # there were no padding, and halves whatever comes out
            o = t >> 1
            return o, (k[None] % 2 == i[:, None] % 2) & (t >= 0) & (o < O)
        o = torch.div(t, S, rounding_mode="floor")
        return o, (t >= 0) & (t % S == 0) & (o < O)

    oh, vh = axis(ih, kh, PH, SH, c.OH)
    ow, vw = axis(iw, kw, PW, SW, c.OW)
    valid = vh & vw
    if last_short:
        valid &= ~((ih == c.H - 1)[:, None] & (oh == c.OH - 1))
    npix = c.N * c.OH * c.OW
    pix = ((n[:, None] * c.OH + oh) * c.OW + ow).clamp(0, npix - 1)
    A = dy.reshape(npix, c.Cout)[pix]
    return (A * valid[..., None]).reshape(gm.numel(), c.T * c.Cout)


_DECODES = {"swap_hw": "swap_hw", "swap_p": "swap_p", "swap_s": "swap_s",
            "swap_k": "swap_k"}


def _operands(c, inp, direction, variant):
    """canonical A [P, R], B [R, Q] of one direction under a wrong decode"""
    opt = {_DECODES[variant]: True} if variant in _DECODES else {}
    w = inp.w
    if variant == "w_untransposed":
        w = w.transpose(2, 3)
    if direction == "fwd":
        if variant == "pad_wrap":
            opt["wrap"] = True
        return fwd_gather(c, inp.x, **opt), w.reshape(c.K, c.Cout)
    if direction == "dgrad":
        if variant == "parity_start_nopad":
            opt["start_nopad"] = True
        if variant == "dgrad_last_short":
            opt["last_short"] = True
        return (dgrad_gather(c, inp.dy, **opt),
                w.permute(0, 1, 3, 2).reshape(c.Rd, c.Cin))
    if direction == "wgrad":
        if variant == "pad_wrap":
            opt["wrap"] = True
        return fwd_gather(c, inp.x, **opt).t(), inp.dy.reshape(c.M, c.Cout)
    # db: the wgrad GEMM's extra row, x == 1
    return torch.ones(1, c.M, dtype=torch.float64), \
        inp.dy.reshape(c.M, c.Cout)


def _dropped_rows(c, direction, variant):
    R = {"fwd": c.K, "dgrad": c.Rd, "wgrad": c.M, "db": c.M}[direction]
    if variant == "drop_last_k":
        return [R - 1]
    if variant == "drop_ragged_chunk":
        return list(range(R - R % 64, R))
    if variant == "split_row" and direction in ("wgrad", "db"):
        return [R // 2]
    if variant == "bias_row_short" and direction == "db":
        return list(range(R - ((R - 1) % 64 + 1), R))
    return []


@functools.lru_cache(maxsize=6)
def _product(c, layer, direction, variant, absolute=False):
    """A @ B of one direction in float64 under one wrong rule"""
    inp = inputs(c, layer)
    if absolute:
        inp = inp.abs()
    A, B = _operands(c, inp, direction, variant)
    rows = _dropped_rows(c, direction, variant)
    if rows:
        keep = torch.ones(A.shape[1], dtype=torch.bool)
        keep[rows] = False
        A, B = A[:, keep], B[keep]
    if variant == "slab_bf16":
        h = A.shape[1] // 2
        return bf(A[:, :h] @ B[:h]) + bf(A[:, h:] @ B[h:])
    pre = A @ B
    return bf(pre) if variant == "acc_bf16" else pre


def _reshape(c, direction, out):
    if direction == "fwd":
        return out.reshape(c.N, c.OH, c.OW, c.Cout)
    if direction == "dgrad":
        return out.reshape(c.N, c.H, c.W, c.Cin)
    if direction == "wgrad":
        return out.reshape(c.KH, c.KW, c.Cin, c.Cout)
    return out.reshape(c.Cout)


def _stats_of(y):
    return torch.stack([y.sum(dim=(0, 1, 2)), (y * y).sum(dim=(0, 1, 2))])


def ref64(c, layer, key, variant=None):
    """float64 result of one output under one wrong rule (None: the right
    one)"""
    direction = KEYS[key][0]
    inp = inputs(c, layer)
    out = _reshape(c, direction, _product(c, layer, direction, variant))
    if direction == "dgrad" and variant == "parity_class_zero":
        # the class that always has a tap (start_h == start_w == 0)
        out = out.clone()
        out[:, c.PH % 2::2, c.PW % 2::2] = 0
    if direction != "fwd":
        return out
    if variant == "bias_by_pixel":
        bias = inp.bias[torch.arange(c.OW) % c.Cout][None, None, :, None]
    else:
        bias = inp.bias
    if key == "y_relu":
        if variant == "relu_before_bias":
            return out.clamp_min(0) + bias
        return (out + bias).clamp_min(0)
    y = out + bias
    if key != "stats":
        return y
    if variant == "stats_rounded":
        y = y.to(c.dtype).double()
    return _stats_of(y)


@functools.lru_cache(maxsize=None)
def big_y(c):
    """some |y| of layer 1 is above 256: its bf16 rounding is not exact"""
    return "y" in c.keys and ref64(c, 1, "y").abs().max().item() > 256


def _dir(key):
    return KEYS[key][0]


def _has_pad_wrap(c):
    return c.PW > 0 or (c.PH > 0 and c.N > 1)


# layer-1 wrong rules: name -> applies(case, key)
VARIANTS1 = {
    "drop_last_k": lambda c, k: True,
    "drop_ragged_chunk": lambda c, k: c.R(k) % 64 != 0,
    "swap_hw": lambda c, k: (_dir(k) in ("fwd", "wgrad") and c.OH != c.OW)
    or (_dir(k) == "dgrad" and c.H != c.W),
    "swap_p": lambda c, k: _dir(k) != "db" and c.PH != c.PW,
    "swap_s": lambda c, k: _dir(k) != "db" and c.SH != c.SW,
    "swap_k": lambda c, k: _dir(k) != "db" and c.KH != c.KW,
    "pad_wrap": lambda c, k: _dir(k) in ("fwd", "wgrad") and _has_pad_wrap(c),
    "parity_class_zero": lambda c, k: k == "dx" and c.SH == 2 and c.SW == 2,
    "parity_start_nopad": lambda c, k: k == "dx" and c.SH == 2 and c.SW == 2
    and (c.PH % 2 == 1 or c.PW % 2 == 1),
    "dgrad_last_short": lambda c, k: k == "dx"
    and _last_short_tap(c) is not None,
    "bias_by_pixel": lambda c, k: _dir(k) == "fwd",
    "relu_before_bias": lambda c, k: k == "y_relu",
    "stats_rounded": lambda c, k: k == "stats" and c.dtype == BF16
    and big_y(c),
    "bias_row_short": lambda c, k: _dir(k) == "db",
    "split_row": lambda c, k: _dir(k) in ("wgrad", "db") and c.M >= 2,
    "w_untransposed": lambda c, k: _dir(k) in ("fwd", "dgrad")
    and c.Cin == c.Cout,
}


def exact_ref(c, key, variant=None):
    return ref64(c, 1, key, variant).to(c.out_dtype(key))


def exact_conditions(c):
    """asserts the layer-1 conditions of one case; returns (max S, max
    sum |y|, max sum y^2)"""
    inp = inputs(c, 1)
    for t in (inp.x, inp.w, inp.dy, inp.bias):
        assert (t != 0).all() and (t == t.round()).all(), c
    smax = 0.0
    for direction in ("fwd", "dgrad", "wgrad", "db"):
        if not any(_dir(k) == direction for k in c.keys):
            continue
        S = _product(c, 1, direction, None, True)
        if direction == "fwd":
            S = S + inp.bias.abs()
        smax = max(smax, S.max().item())
    assert smax < 2 ** 24, (c, smax)
    sabs = ssq = 0.0
    if "stats" in c.keys:
        y = ref64(c, 1, "y")
        sabs = y.abs().sum(dim=(0, 1, 2)).max().item()
        ssq = (y * y).sum(dim=(0, 1, 2)).max().item()
        assert sabs < 2 ** 24 and ssq < 2 ** 24, (c, sabs, ssq)
    return smax, sabs, ssq


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def honest(c, layer, key, dtype=torch.float32):
    """torch's own convolution on the CPU in `dtype` (fp32: the honest model
    of a kernel; float64: a second opinion on the reference), rounded once to
    the output dtype; the statistics from the unrounded y"""
    inp = inputs(c, layer)
    x, dy = _nchw(inp.x.to(dtype)), _nchw(inp.dy.to(dtype))
    w = inp.w.to(dtype).permute(3, 2, 0, 1)          # [Cout, Cin, KH, KW]
    stride, pad = (c.SH, c.SW), (c.PH, c.PW)
    direction = _dir(key)
    if direction == "fwd":
        y = F.conv2d(x, w, inp.bias.to(dtype), stride, pad).permute(0, 2, 3, 1)
        if key == "y_relu":
            y = y.clamp_min(0)
        out = _stats_of(y) if key == "stats" else y
    elif direction == "dgrad":
        out = torch.nn.grad.conv2d_input(x.shape, w, dy, stride,
                                         pad).permute(0, 2, 3, 1)
    elif direction == "wgrad":
        out = torch.nn.grad.conv2d_weight(x, w.shape, dy, stride,
                                          pad).permute(2, 3, 1, 0)
    else:
        out = dy.sum(dim=(0, 2, 3))
    return out.to(c.out_dtype(key))


def check_exact(got, c, key):
    """0.0 when got equals the exact reference bit for bit, else the
    largest difference (inf for a NaN, e.g. from a guard band)"""
    want = exact_ref(c, key)
    got = got.detach().cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, \
        (key, got.dtype, got.shape, want.dtype, want.shape)
    if torch.equal(got, want):
        return 0.0
    d = (got.double() - want.double()).abs()
    return float("inf") if torch.isnan(d).any() else d.max().item()


# ---------------------------------------------------------------------------
# layer 2: bound and wrong variants
# ---------------------------------------------------------------------------

class Ref2:
    """float64 reference of one layer-2 output with its element-wise bound
    and the plain worst-case form `bound_plain` (2 R u S + 2^-7 |ref|)"""

    def __init__(self, c, key):
        direction = _dir(key)
        inp = inputs(c, 2)
        self.out = ref64(c, 2, key)
        R = c.R(key)
        S = _reshape(c, direction, _product(c, 2, direction, None, True))
        if direction == "fwd":
            S = S + inp.bias.abs()
        acc = lambda r: min(ACC * r ** 0.5, 2 * r) * U
        if key == "stats":
            y = ref64(c, 2, "y")
            d = acc(R) * S + 2 * U * y.abs()
            dp = 2 * R * U * S + 2 * U * y.abs()
            sa, sq = y.abs().sum(dim=(0, 1, 2)), (y * y).sum(dim=(0, 1, 2))

            def fold(d, f):
                return torch.stack([
                    d.sum(dim=(0, 1, 2)) + f * sa,
                    (2 * y.abs() * d + d * d).sum(dim=(0, 1, 2))
                    + (f + U) * sq])
            self.bound = fold(d, acc(c.M)) + 1e-30
            self.bound_plain = fold(dp, 2 * c.M * U) + 1e-30
            return
        tail = 2 * U * self.out.abs() + 1e-30
        self.bound = acc(R) * S + tail
        self.bound_plain = 2 * R * U * S + tail
        if c.out_dtype(key) == BF16:
            self.bound_plain = self.bound_plain + BF16_ULP * self.out.abs()


@functools.lru_cache(maxsize=None)
def ref2(c, key):
    return Ref2(c, key)


def _ratio(got, c, key, bound):
    r = ref2(c, key)
    assert got.shape == r.out.shape, (key, got.shape, r.out.shape)
    g = got.double()
    err = (g - r.out).abs()
    if got.dtype == BF16:
        # got = round-to-nearest of some v with |got - v| <= half the bf16
        # spacing at got: only the rest of the distance is v's own error
        err = (err - bf16_spacing(g) / 2).clamp_min(0)
    ratio = err / bound
    return float("inf") if torch.isnan(ratio).any() else ratio.max().item()


def check_bound(got, c, key):
    """worst err / bound of a layer-2 output (inf for a NaN)"""
    got = got.detach().cpu()
    assert got.dtype == c.out_dtype(key), (key, got.dtype)
    return _ratio(got, c, key, ref2(c, key).bound)


# layer-2 wrong rules: name -> applies(case, key)
VARIANTS2 = {
    # two half-R slabs rounded to bf16 before the fold
    "slab_bf16": lambda c, k: k in ("y", "dx", "dw_f32", "dw_dt", "db_f32"),
    # accumulator rounded to bf16 before the epilogue; a bf16 output rounds
    # the same value again and hides it
    "acc_bf16": lambda c, k: k != "stats" and c.out_dtype(k) == F32,
    # statistics from the bf16-rounded y
    "stats_rounded": lambda c, k: k == "stats" and c.dtype == BF16,
}


def variant2_distance(c, key, name, plain=False):
    """err / bound of a wrong variant's result, rounded to the output dtype
    as a kernel would deliver it; plain=True measures |err| against the
    untightened bound"""
    v = ref64(c, 2, key, name)
    r = ref2(c, key)
    if plain:
        return ((v - r.out).abs() / r.bound_plain).max().item()
    return _ratio(v.to(c.out_dtype(key)), c, key, r.bound)
