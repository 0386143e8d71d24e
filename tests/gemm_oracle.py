"""Oracle for the GEMM family (gemm.hip, bmm.hip): case tables, inputs,
float64 references, bounds, guard bands and wrong variants, shared by
test_gemm_oracle_cpu.py and test_gpu_gemm_oracle.py.

Everything here is torch on the CPU and nothing imports the extension.

Canonical form. Every entry point computes out[P, Q] = sum_r A[p, r] B[r, q]
(per batch for bmm), then an epilogue. The oracle builds A [P, R] and
B [R, Q] and `operands` lays them out the way the entry point wants them:

  gemm, gemm_skinny   a = A [M, K],        b = B [K, N]      R = K
  gemm_nt             a = A [M, K],        b = B^T [N, K]    R = K
  gemm_tn             a = A^T [M, K],      b = B [M, N]      R = M, out [K, N]
  bmm                 a, b per layout (N = natural, T = transpose view)

Layer 1, exact. A and B hold non-zero integers (+-1, +-2; +-1 alone once R
is large), bias and residual are integers, the activation is linear or
relu. Then S = |A| @ |B| + |bias| + |resid| < 2^24, every partial sum in
any order is an integer below 2^24 and is exact in fp32, and the kernel's
output must equal ref64.to(dtype) bit for bit. For R > 6000 the rows in
[1024, 1024 + 2H), H = (R - 2048) // 2, cancel in pairs H apart (A's
columns repeat, B's rows repeat negated), so the sum is as large as that
of 2048 random terms and a bf16 output keeps integer resolution, while
dropping or doubling fewer than H consecutive rows still changes every
output.

Layer 2, precision. x = randn, w = 0.05 randn, rounded to the dtype; the
reference is float64 from the rounded inputs. The untightened element-wise
bound (Ref2.bound_issue), with u = 2^-24, S the absolute-value twin of the
pre-activation and L the activation's largest slope (1, or 1.13 for
tanh-GELU), is

  L * 2 R u S + A_ACT + 2 u (|act| + |resid|) + 2^-7 |ref| (bf16) + 1e-30
  [+ L (1e-4 S_ln  (+ 2^-8 S_ln in the bf16 MFMA skinny form))]

with S_ln = |LN64(x)| @ |w| + |bias|, 1e-4 the relative invstd tolerance
docs/KERNELS.md states for every norm site and 2^-8 the bf16 rounding of the
normalised row where the kernel stages it as bf16. Against it the wrong
variants below land as near as 0.06 bounds (slab_bf16), 0.19 (ln_var_km1)
and 0.90 (acc_bf16): the worst-case terms hide them. Ref2.bound is that
bound with each term tightened; it is never larger (asserted on the CPU):

* Output rounding. A bf16 result is the round-to-nearest of some fp32 value
  v, so |got - v| is at most half the bf16 spacing at got. check_bound
  takes exactly that off |got - ref| and holds the rest, v's own error, to
  the bound; the bound has no output term. (Exact at any |ref|, also near
  zero.)
* Accumulation. 2 R u S assumes that all R rounding errors line up. They
  are signed and independent of each other, so they add up like sqrt(R)
  (Higham and Mary, "A new approach to probabilistic rounding error
  analysis", 2019: lambda sqrt(R) u S fails with probability 2 exp(-lambda^2
  / 2), in any summation order). The constant is measured, as the attention
  oracle's is: the honest fp32 model's worst err / (sqrt(R) u S) over the
  fp32-output cases is ACC_FLOOR = 0.7 (re-measured by the CPU test), times
  ACC_FACTOR = 4 for the kernels' other summation orders; capped at 2 R.
* Activation. A pre-activation error d comes out of the GELU as at most
  (|gelu'(pre)| + GELU_CURV d / 2) d, capped at L d.
* LayerNorm statistics. An invstd off by eps scales ln - beta, so the
  product moves by eps times the SIGNED sum (ln64 - beta) @ w: the term is
  1e-4 |(ln64 - beta) @ w|, not 1e-4 S_ln.
* bf16 normalised row (MFMA skinny form). The reference rounds its float64
  normalised row to bf16 as the kernel does, and the bound pays only for
  roundings that can flip: see _flip_term.

A_ACT is the activation's own evaluation error: the largest difference
between common.h::act_apply's tanh-GELU formula evaluated in fp32 and in
float64 on the layer-2 pre-activations, A_ACT_MEASURED (printed and
re-measured by test_gemm_oracle_cpu.py), times A_ACT_FACTOR = 4 because the
device tanhf is not the host's.

Wrong variants. Layer 1: every one is unequal on every case it applies to.
Layer 2: each must land TEETH = 3 bounds away on every case it applies to;
the smallest distances measured by test_gemm_oracle_cpu.py (MEASURED_TEETH)
are

  slab_bf16 5.51   acc_bf16 14.78   ln_var_km1 3.13
  ln_no_beta 4881   ln_gamma_shift 12185

slab_bf16 applies to every case, acc_bf16 to every fp32 output (a bf16
output rounds the same value again and hides it), the LN variants to every
fused-LN case, ln_var_km1 in fp32 (the bf16 MFMA form's own row rounding is
coarser than 1 / (2K)). ln_var_km1 cannot clear much more than 3 at K =
1030: it changes invstd by 4.9e-4 and the stated tolerance is 1e-4.
"""

import functools

import torch

BF16, F32 = torch.bfloat16, torch.float32
U = 2.0 ** -24
BF16_ULP = 2.0 ** -7           # as in test_gpu_wgrad_bias.py
GUARD = 4096                    # NaN elements on each side of an operand
LN_EPS = 1e-5
GELU_SLOPE = 1.13               # max |d gelu_tanh / dx| = 1.129
ACT = {"linear": 0, "relu": 1, "gelu": 2}

A_ACT_MEASURED = 4.3e-7         # see the docstring; asserted by the CPU test
A_ACT_FACTOR = 4.0
A_ACT = A_ACT_FACTOR * A_ACT_MEASURED
LN_STATS_TOL = 1e-4
LN_BF16_ROW = 2.0 ** -8
TEETH = 3.0                     # layer-2 variants must reach TEETH bounds
GELU_CURV = 1.2                 # max |gelu_tanh''| = 1.13 (at x = 0: 0.80)
# fp32 accumulation: largest err / (sqrt(R) u S) of the honest fp32 model on
# the fp32-output cases (measured, asserted by the CPU test), times a factor
# for the kernels' other summation orders
ACC_FLOOR = 0.7
ACC_FACTOR = 4.0

# smallest measured distance per layer-2 variant (CPU, this module's cases)
MEASURED_TEETH = {"slab_bf16": 5.51, "acc_bf16": 14.78, "ln_no_beta": 4881.5,
                  "ln_gamma_shift": 12185.0, "ln_var_km1": 3.13}

# layer-1 epilogues: (bias, activation, residual: None / "any" / "neg")
EPILOGUES = {
    "none": (False, "linear", None),
    "bias": (True, "linear", None),
    "relu": (True, "relu", None),
    "lin_res": (True, "linear", "any"),
    "relu_res": (True, "relu", "neg"),
}
EP_ALL = tuple(EPILOGUES)
EP_NORES = ("none", "bias", "relu")
EP_NONE = ("none",)


def dt_name(dt):
    return "bf16" if dt == BF16 else "f32"


class Case:
    """One shape on one route. M, N, K are the entry point's own."""

    def __init__(self, entry, route, dtype, M, N, K, *, layers=(1, 2),
                 eps=EP_NONE, unaligned=(), ln=False, out_in_dt=True,
                 batch=None, layout="NN", noncontig=False, env32=True):
        self.entry, self.route, self.dtype = entry, route, dtype
        self.M, self.N, self.K = M, N, K
        self.layers, self.eps = tuple(layers), tuple(eps)
        self.unaligned = tuple(unaligned)
        self.ln, self.out_in_dt = ln, out_in_dt
        self.batch, self.layout, self.noncontig = batch, layout, noncontig
        self.env32 = env32
        if entry == "gemm_tn":
            self.P, self.R, self.Q = K, M, N
        else:
            self.P, self.R, self.Q = M, K, N
        self.out_dtype = dtype if (entry != "gemm_tn" or out_in_dt) else F32
        self.has_ep = entry in ("gemm", "gemm_skinny")
        # the bf16 MFMA skinny form stages the (normalised) row as bf16
        self.mfma_skinny = (entry == "gemm_skinny" and dtype == BF16 and M > 4)
        self.nsplit = self._nsplit()

    def _nsplit(self):
        """K slices of the route, where the oracle knows them (the first
        row of the second slice is one of the layer-1 variants)."""
        if self.entry == "gemm_skinny":      # gemm.hip::gemm_skinny_nsplit
            ncb = -(-self.N // (64 if self.mfma_skinny else 128))
            ns = max(1, min(32, 512 // ncb))
            return max(2, min(ns, max(1, self.K // 32)))
        return 2

    @property
    def id(self):
        s = f"{self.entry}-{dt_name(self.dtype)}-{self.route}-" \
            f"{self.M}x{self.N}x{self.K}"
        if self.batch:
            s += f"-b{self.batch}{self.layout}"
        if self.entry == "gemm_tn":
            s += "-outdt" if self.out_in_dt else "-outf32"
        if self.ln:
            s += "-ln"
        if self.unaligned:
            s += "-unal_" + "".join(self.unaligned)
        return s

    def __repr__(self):
        return self.id

    @property
    def seed(self):
        return (hash_str(self.id) % (2 ** 31 - 1)) + 1


def hash_str(s):
    h = 1469598103934665603
    for ch in s.encode():
        h = ((h ^ ch) * 1099511628211) % (2 ** 64)
    return h


# ---------------------------------------------------------------------------
# case tables
# ---------------------------------------------------------------------------

def _dense_cases():
    routes = [
        (BF16, 128, 64, 64, "nt32_z1"),
        (BF16, 128, 64, 256, "nt32_z2_splitk_fin_ep"),
        (BF16, 128, 66, 256, "nt32_z1_raggedN"),
        (BF16, 130, 70, 264, "nt32_raggedMN"),
        (BF16, 32, 64, 64, "k_gemm_nn_glds"),
        (BF16, 100, 10, 27, "k_gemm_nn_scalar"),
        (BF16, 1, 65, 100, "gemv_nn1_unsplit"),
        (BF16, 1, 768, 768, "gemv_nn1_split_fin2"),
        (F32, 128, 64, 256, "nt_z_zf2_splitk_fin_ep"),
        (F32, 128, 64, 64, "nt_db"),
        (F32, 128, 66, 3080, "k_gemm_nt_glds_longK"),
        (F32, 32, 64, 64, "k_gemm_nn_glds"),
        (F32, 100, 10, 27, "k_gemm_nn_scalar"),
        (F32, 1, 65, 100, "gemv_nn1_unsplit"),
        (F32, 1, 768, 768, "gemv_nn1_split_fin2"),
    ]
    out = [Case("gemm", r, dt, M, N, K, eps=EP_ALL,
                layers=(1, 2) if K <= 1100 else (1,))
           for dt, M, N, K, r in routes]
    for dt in (BF16, F32):    # M = 1, K > 8192: no residual on this route
        out.append(Case("gemm", "gemv_hugeK", dt, 1, 65, 8200, eps=EP_NORES,
                        layers=(1,)))
    # M >= 64 off the vec_ok route: K % 8 != 0, and an unaligned A
    out.append(Case("gemm", "k_gemm_nn_K%8", BF16, 128, 64, 260, eps=EP_ALL))
    out.append(Case("gemm", "k_gemm_nn_unalignedA", BF16, 128, 64, 256,
                    eps=EP_ALL, unaligned=("a",)))
    out.append(Case("gemm", "k_gemm_nn_unalignedA", F32, 128, 64, 256,
                    eps=EP_ALL, unaligned=("a",)))
    return out


# bf16 16x16-tile routes, reachable only with TNN_GEMM32=0 (one child process)
def _gemm16_cases():
    out = [Case("gemm", r, BF16, M, N, K, eps=EP_ALL, env32=False,
                layers=(1, 2) if K <= 1100 else (1,))
           for M, N, K, r in [(128, 64, 64, "nt_db16"),
                              (128, 64, 256, "nt_z16_splitk_fin_ep"),
                              (128, 66, 3080, "k_gemm_nt_glds16_longK")]]
    out.append(Case("gemm_nt", "nt_z16_splitk_reduce", BF16, 128, 64, 512,
                    env32=False))
    return out


def _nt_cases():
    out = []
    for dt, M, N, K, r in [
            (BF16, 128, 64, 512, "nt32_split"),
            (F32, 128, 64, 512, "nt_z_splitk_reduce"),
            (BF16, 64, 27, 130, "k_gemm_nt_scalar"),
            (F32, 64, 27, 130, "k_gemm_nt_scalar"),
            (BF16, 1, 100, 33, "gemv_nt"),
            (F32, 1, 100, 33, "gemv_nt"),
            (BF16, 64, 64, 64, "square"),
            (F32, 64, 64, 64, "square")]:
        out.append(Case("gemm_nt", r, dt, M, N, K))
    for dt in (BF16, F32):
        # B off 16-byte alignment with K a vector multiple: row staging
        # must not take the 16-byte DMA form
        out.append(Case("gemm_nt", "k_gemm_nt_unalignedB", dt, 128, 64, 64,
                        unaligned=("b",)))
        out.append(Case("gemm_nt", "gemv_nt_unalignedB", dt, 1, 100, 32,
                        unaligned=("b",)))
        out.append(Case("gemm_nt", "hugeK_split", dt, 256, 128, 16384,
                        layers=(1,)))
    return out


def _tn_cases():
    out = []
    for dt in (F32, BF16):
        for oid in (False, True):
            for M, N, K, r in [(512, 64, 128, "vec_slabs"),
                               (130, 33, 27, "scalar_kernel_scalar_reduce"),
                               (4096, 64, 64, "splitk_fold"),
                               (256, 64, 128, "splitk_reduce4")]:
                out.append(Case("gemm_tn", r, dt, M, N, K, out_in_dt=oid,
                                layers=(1, 2) if M <= 1100 else (1,)))
        out.append(Case("gemm_tn", "unalignedA", dt, 512, 64, 128,
                        unaligned=("a",)))
    return out


SKINNY_M = (1, 2, 3, 4, 5, 8, 9, 13, 16)


def _skinny_cases():
    out = []
    seen = set()

    def add(dt, M, N, K, route, **kw):
        c = Case("gemm_skinny", route, dt, M, N, K, eps=EP_ALL, **kw)
        if c.id not in seen:
            seen.add(c.id)
            out.append(c)

    for dt in (F32, BF16):
        # every M, three slices at unaligned k (0, 33, 66), odd and even N
        for M in SKINNY_M:
            add(dt, M, 65, 100, "slices_0_33_66_oddN", layers=(1,))
            add(dt, M, 66, 100, "slices_0_33_66_evenN", layers=(1,))
        for M in (3, 9, 16):
            # N % 64 in {0, 1, 2, 63}, N = 1, N = 2
            for N in (1, 2, 64, 127):
                add(dt, M, N, 100, f"N%64={N % 64}", layers=(1,))
            add(dt, M, 64, 17, "one_slice_K17", layers=(1,))
            add(dt, M, 130, 61, "one_slice_K61_batch_tail", layers=(1,))
            # weight pointer only element-aligned at even N: element loads
            add(dt, M, 64, 100, "evenN_unalignedB", layers=(1,),
                unaligned=("b",))
            add(dt, M, 66, 100, "unalignedX", layers=(1,), unaligned=("a",))
    # one slice, more than one LDS chunk, ragged last chunk
    # MFMA form: chunks of 1024 + 6, even N (dword feed) and odd N
    add(BF16, 16, 16450, 1030, "mfma_chunks_1024+6_evenN", layers=(1,))
    add(BF16, 9, 16451, 1030, "mfma_chunks_1024+6_oddN", layers=(1,))
    # VALU form: chunks of 512 + 8, and two slices of 515 = 512 + 3
    add(F32, 3, 32800, 520, "valu_chunks_512+8", layers=(1,))
    add(BF16, 4, 21801, 1030, "valu_2slices_515_oddN", layers=(1,))
    # MFMA two-step batch loop (ks + 64 < kc_n) and its tail: one slice
    # (N wide enough for nsplit = 1) of each length around the thresholds
    for K in (64, 65, 112, 113, 129, 200):
        add(BF16, 16, 16450, K, "mfma_one_slice_batch_edge", layers=(1,))
    # LN row cache threshold (SK_LN_RC * 64 = 1024) and split shapes: both
    # layers; layer 2 runs them with and without the fused LN
    for dt in (F32, BF16):
        for M in (3, 16):
            for K in (100, 1024, 1025, 1030):
                for N in (65, 768):
                    add(dt, M, N, K, "ln_edge")
    return out


def _skinny_ln_cases():
    return [Case("gemm_skinny", c.route, c.dtype, c.M, c.N, c.K, eps=EP_ALL,
                 layers=(2,), ln=True)
            for c in _skinny_cases() if 2 in c.layers]


def _gemv_ln_cases():
    return [Case("gemm", "gemv_nn1_ln", dt, 1, N, K, eps=EP_ALL, layers=(2,),
                 ln=True)
            for dt in (F32, BF16) for K in (100, 768, 1030)
            for N in (65, 768)]


BMM_SHAPES = [(6, 64, 64, 64), (4, 128, 96, 64), (3, 57, 130, 33),
              (2, 512, 512, 64), (12, 1, 64, 64)]


def _bmm_cases():
    out = []
    for dt in (F32, BF16):
        for (B, M, N, K) in BMM_SHAPES:
            for lay in ("NN", "NT", "TN", "TT"):
                l2 = (B, M, N, K) == BMM_SHAPES[2] and lay == "NT"
                out.append(Case("bmm", "layout", dt, M, N, K, batch=B,
                                layout=lay, layers=(1, 2) if l2 else (1,)))
        out.append(Case("bmm", "noncontig_fallback", dt, 64, 32, 64, batch=2,
                        noncontig=True, layers=(1,)))
    return out


CASES = (_dense_cases() + _nt_cases() + _tn_cases() + _skinny_cases()
         + _skinny_ln_cases() + _gemv_ln_cases() + _bmm_cases())
GEMM16_CASES = _gemm16_cases()
ALL_CASES = CASES + GEMM16_CASES
assert len({c.id for c in ALL_CASES}) == len(ALL_CASES)


def cases_for(layer, entries=None, env32=True):
    return [c for c in ALL_CASES if layer in c.layers and c.env32 == env32
            and (entries is None or c.entry in entries)]


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------

def _signs(shape, g):
    return torch.randint(0, 2, shape, generator=g, dtype=torch.int64) * 2 - 1


def _ints(shape, mags, g):
    m = torch.tensor(mags)[torch.randint(0, len(mags), shape, generator=g)]
    return (_signs(shape, g) * m).double()


class Inputs1:
    """layer-1 operands in canonical form, float64 holding integers"""

    def __init__(self, c):
        g = torch.Generator().manual_seed(c.seed)
        bs = (c.batch,) if c.batch else ()
        R = c.R
        amag = (1, 2) if R <= 3100 else (1,)
        bmag = (1, 2) if R <= 1100 else (1,)
        self.A = _ints(bs + (c.P, R), amag, g)
        self.B = _ints(bs + (R, c.Q), bmag, g)
        if R > 6000:      # rows cancelling in pairs H apart; see the docstring
            lo, H = 1024, (R - 2048) // 2
            self.A[..., lo + H:lo + 2 * H] = self.A[..., lo:lo + H]
            self.B[..., lo + H:lo + 2 * H, :] = -self.B[..., lo:lo + H, :]
        self.bias = _ints((c.Q,), (1, 2, 3, 5, 8), g)
        self.resid_any = _ints((c.P, c.Q), tuple(range(1, 10)), g)
        self.resid_neg = -_ints((c.P, c.Q), tuple(range(1, 10)), g).abs()

    def resid(self, kind):
        return {None: None, "any": self.resid_any, "neg": self.resid_neg}[kind]


class Inputs2:
    """layer-2 operands in canonical form, float64 holding dtype values"""

    def __init__(self, c):
        g = torch.Generator().manual_seed(c.seed + 1)
        bs = (c.batch,) if c.batch else ()
        rd = lambda t: t.to(c.dtype).double()
        self.A = rd(torch.randn(bs + (c.P, c.R), generator=g))
        self.B = rd(0.05 * torch.randn(bs + (c.R, c.Q), generator=g))
        self.bias = rd(0.5 * torch.randn(c.Q, generator=g))
        self.resid = rd(torch.randn(c.P, c.Q, generator=g))
        # fp32 LayerNorm parameters
        self.gamma = (1 + 0.3 * torch.randn(c.R, generator=g)).float()
        self.beta = (0.3 * torch.randn(c.R, generator=g)).float()


@functools.lru_cache(maxsize=None)
def inputs1(c):
    return Inputs1(c)


@functools.lru_cache(maxsize=None)
def inputs2(c):
    return Inputs2(c)


def operands(c, A, B):
    """canonical A, B -> the entry point's contiguous (a, b); bmm's layouts
    are made in device_args"""
    if c.entry == "gemm_nt":
        return A, B.transpose(-1, -2).contiguous()
    if c.entry == "gemm_tn":
        return A.transpose(-1, -2).contiguous(), B
    return A, B


def guarded(t, dtype, device, unaligned=False):
    """a contiguous copy of t inside a NaN-filled buffer with at least GUARD
    elements on each side. The view starts GUARD elements in (a multiple of
    16 bytes), or GUARD + 1 (an odd element count) for an unaligned one."""
    off = GUARD + (1 if unaligned else 0)
    buf = torch.full((t.numel() + 2 * GUARD + 8,), float("nan"), dtype=dtype)
    buf[off:off + t.numel()] = t.reshape(-1).to(dtype)
    buf = buf.to(device)
    v = buf[off:off + t.numel()].view(t.shape)
    if device != "cpu" and device != torch.device("cpu"):
        assert (v.data_ptr() % 16 == 0) != unaligned, "guard band alignment"
    return v


def device_args(c, inp, device, ep="none", layer=1):
    """guard-banded call arguments for the case's entry point:
    (a, b, bias, act_kind, residual, ln_gamma, ln_beta)"""
    dt = c.dtype
    ua = lambda name: name in c.unaligned
    if c.entry == "bmm":
        A, B = inp.A, inp.B
        if c.noncontig:
            # a is every other column of a twice-as-wide buffer
            wide = torch.zeros(A.shape[:-1] + (2 * A.shape[-1],),
                               dtype=torch.float64)
            wide[..., ::2] = A
            a = guarded(wide, dt, device)[..., ::2]
        elif c.layout[0] == "T":
            a = guarded(A.transpose(-1, -2).contiguous(), dt,
                        device).transpose(-1, -2)
        else:
            a = guarded(A, dt, device)
        if c.layout[1] == "T":
            b = guarded(B.transpose(-1, -2).contiguous(), dt,
                        device).transpose(-1, -2)
        else:
            b = guarded(B, dt, device)
        return a, b, None, 0, None, None, None
    a, b = operands(c, inp.A, inp.B)
    a = guarded(a, dt, device, ua("a"))
    b = guarded(b, dt, device, ua("b"))
    if not c.has_ep:
        return a, b, None, 0, None, None, None
    if layer == 1:
        has_bias, act, rk = EPILOGUES[ep]
        bias = inp.bias if has_bias else None
        resid = inp.resid(rk)
    else:
        bias, act, resid = inp.bias, "gelu", inp.resid
    bias = None if bias is None else guarded(bias, dt, device)
    resid = None if resid is None else guarded(resid, dt, device)
    g = be = None
    if c.ln:
        g = guarded(inp.gamma, F32, device)
        be = guarded(inp.beta, F32, device)
    return a, b, bias, ACT[act], resid, g, be


# ---------------------------------------------------------------------------
# layer 1: exact reference and wrong variants
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=8)
def _product1(c):
    inp = inputs1(c)
    return inp.A @ inp.B


def _without_rows(c, rows):
    """the product with the terms of the k rows `rows` left out"""
    inp = inputs1(c)
    return _product1(c) - inp.A[..., rows] @ inp.B[..., rows, :]


def exact_ref(c, ep="none", variant=None):
    """float64 result (integers) of one layer-1 epilogue; `variant` names a
    wrong rule from VARIANTS1"""
    inp = inputs1(c)
    has_bias, act, rk = EPILOGUES[ep]
    bias = inp.bias if has_bias else None
    resid = inp.resid(rk)
    R, P, Q = c.R, c.P, c.Q
    if variant == "drop_last_k":
        pre = _without_rows(c, [R - 1])
    elif variant == "drop_k_tail":
        t = R % 16 or R % 64
        pre = _without_rows(c, list(range(R - t, R)))
    elif variant == "drop_slice_row":
        pre = _without_rows(c, [R // c.nsplit])
    elif variant == "b_untransposed":
        pre = inp.A @ inp.B.transpose(-1, -2)
    else:
        pre = _product1(c).clone()
    if variant == "row_from_prev":
        pre[..., P - 1, :] = pre[..., P - 2, :]
    elif variant == "swap_col_pairs":
        idx = torch.arange(Q)
        sw = idx ^ 1
        sw[sw >= Q] = Q - 1
        pre = pre[..., sw]
    elif variant == "last_col_from_prev":
        pre[..., Q - 1] = pre[..., Q - 2]
    if bias is not None:
        if variant == "bias_by_row":
            pre = pre + bias[torch.arange(P) % Q][:, None]
        else:
            pre = pre + bias
    if resid is not None:
        if variant == "resid_stride":
            flat = resid.reshape(-1)
            i = torch.arange(P)[:, None] * (Q + 1) + torch.arange(Q)[None, :]
            resid = flat[i % flat.numel()]
        if variant == "resid_before_act":
            pre = pre + resid
            resid = None
    out = pre.clamp_min(0) if act == "relu" else pre
    return out if resid is None else out + resid


def _linear(ep):
    return EPILOGUES[ep][1] == "linear"


# name -> applies(case, epilogue)
VARIANTS1 = {
    "drop_last_k": lambda c, ep: True,
    "drop_k_tail": lambda c, ep: (c.R % 16 or c.R % 64) != 0,
    "drop_slice_row": lambda c, ep: c.R >= 2,
    # one wrong row or column: under a relu the right and the wrong value
    # can both clip to zero on so few elements, so linear epilogues only
    "row_from_prev": lambda c, ep: c.P >= 2 and _linear(ep),
    "swap_col_pairs": lambda c, ep: c.Q >= 2,
    "last_col_from_prev": lambda c, ep: c.Q >= 2 and _linear(ep),
    "bias_by_row": lambda c, ep: EPILOGUES[ep][0] and c.P >= 2 and c.Q >= 2,
    "resid_before_act": lambda c, ep: ep == "relu_res",
    "resid_stride": lambda c, ep: EPILOGUES[ep][2] is not None and c.P >= 2,
    "b_untransposed": lambda c, ep: c.entry == "gemm_nt" and c.R == c.Q,
}


def exact_conditions(c):
    """the layer-1 conditions of one case: (max S, all non-zero, fraction
    of |ref| <= 256 over the case's epilogues)"""
    inp = inputs1(c)
    S = inp.A.abs() @ inp.B.abs() + inp.bias.abs() + inp.resid_any.abs()
    nonzero = bool((inp.A != 0).all() and (inp.B != 0).all())
    frac = min(((exact_ref(c, ep).abs() <= 256).double().mean().item())
               for ep in c.eps)
    return S.max().item(), nonzero, frac


def honest_exact(c, ep):
    """fp32 torch on the CPU, rounded to the output dtype"""
    inp = inputs1(c)
    has_bias, act, rk = EPILOGUES[ep]
    v = inp.A.float() @ inp.B.float()
    if has_bias:
        v = v + inp.bias.float()
    if act == "relu":
        v = v.clamp_min(0)
    if rk:
        v = v + inp.resid(rk).float()
    return v.to(c.out_dtype)


def check_exact(got, c, ep="none"):
    """0.0 when got equals the exact reference bit for bit, else the
    largest difference (inf for a NaN, e.g. from a guard band)"""
    want = exact_ref(c, ep).to(c.out_dtype)
    got = got.detach().cpu()
    assert got.dtype == c.out_dtype and got.shape == want.shape, \
        (got.dtype, got.shape, want.shape)
    if torch.equal(got, want):
        return 0.0
    d = (got.double() - want.double()).abs()
    return float("inf") if torch.isnan(d).any() else d.max().item()


# ---------------------------------------------------------------------------
# layer 2: float64 reference, bound, honest model and wrong variants
# ---------------------------------------------------------------------------

def gelu_formula(x):
    """common.h::act_apply ACT_GELU, in x's precision"""
    c = 0.7978845608028654
    return 0.5 * x * (1.0 + torch.tanh(c * (x + 0.044715 * x * x * x)))


def ln64(x, gamma, beta, *, no_beta=False, gamma_shift=False, var_km1=False):
    K = x.shape[-1]
    mu = x.mean(-1, keepdim=True)
    d = x - mu
    var = d.pow(2).sum(-1, keepdim=True) / (K - 1 if var_km1 else K)
    g = gamma.double()
    if gamma_shift:
        g = torch.roll(g, 1)
    y = d / torch.sqrt(var + LN_EPS) * g
    return y if no_beta else y + beta.double()


def bf(x):
    return x.to(BF16).to(x.dtype)


def _matmul2(c, A, B, variant):
    if variant == "slab_bf16":
        h = c.R // 2
        return bf(A[..., :h] @ B[..., :h, :]) + bf(A[..., h:] @ B[..., h:, :])
    pre = A @ B
    return bf(pre) if variant == "acc_bf16" else pre


def bf16_spacing(x):
    """distance between neighbouring bf16 numbers at |x| (8 significant
    bits); tiny for x = 0"""
    return torch.exp2(torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -120)))
                      - 7)


class Ref2:
    """float64 reference of a layer-2 case with its bound (element-wise).
    `bound` leaves the output rounding out: check_bound takes that off the
    error exactly. `bound_issue` is the untightened form, for comparison."""

    def __init__(self, c, variant=None):
        inp = inputs2(c)
        A = inp.A
        if c.ln:
            ln = ln64(A, inp.gamma, inp.beta,
                      no_beta=variant == "ln_no_beta",
                      gamma_shift=variant == "ln_gamma_shift",
                      var_km1=variant == "ln_var_km1")
            # the MFMA form stages the normalised row as bf16: so does the
            # reference, and the bound pays only for roundings that can flip
            A = bf(ln) if c.mfma_skinny else ln
        pre = _matmul2(c, A, inp.B, variant)
        S = A.abs() @ inp.B.abs()       # S_ln with a fused LN
        if c.has_ep:
            pre = pre + inp.bias
            S = S + inp.bias.abs()
            act = gelu_formula(pre)
            resid = inp.resid
            self.out = act + resid
            L, a_act = GELU_SLOPE, A_ACT
        else:
            act, resid, self.out = pre, torch.zeros(()), pre
            L, a_act = 1.0, 0.0
        self.pre = pre
        if variant is not None:
            return
        R = c.R
        tail = a_act + 2 * U * (act.abs() + resid.abs()) + 1e-30
        issue = L * 2 * R * U * S
        dpre = min(ACC_FACTOR * ACC_FLOOR * R ** 0.5, 2 * R) * U * S
        if c.ln:
            beta = inp.beta.double()
            issue_ln = LN_STATS_TOL * S
            # invstd off by eps, |eps| <= 1e-4, scales the signed sum G
            stats = LN_STATS_TOL * ((ln - beta) @ inp.B).abs()
            if c.mfma_skinny:
                issue_ln = issue_ln + LN_BF16_ROW * S
                stats = stats + _flip_term(ln, beta, inp.B)
            issue = issue + L * issue_ln
            dpre = dpre + torch.minimum(stats, issue_ln)
        if c.has_ep:
            # a pre-activation error d comes out as at most
            # (|gelu'| + max|gelu''| d / 2) d, and never more than L d
            slope = (gelu_slope(pre).abs() + 0.5 * GELU_CURV * dpre)
            dpre = slope.clamp_max(L) * dpre
        self.bound = dpre + tail
        self.bound_issue = issue + tail
        if c.out_dtype == BF16:
            self.bound_issue = self.bound_issue + BF16_ULP * self.out.abs()


def gelu_slope(x):
    """derivative of gelu_formula (common.h::act_grad's form)"""
    c = 0.7978845608028654
    t = torch.tanh(c * (x + 0.044715 * x * x * x))
    return 0.5 * (1 + t) + 0.5 * x * (1 - t * t) * c * (1 + 3 * 0.044715
                                                          * x * x)


def _flip_term(ln, beta, B):
    """bf16 MFMA skinny form: how far the product can move because the
    kernel's fp32 normalised row rounds to other bf16 numbers than ln64.

    The kernel's row is beta + (1 + eps) (ln - beta) with one eps per row,
    |eps| <= 1e-4, plus fp32 evaluation noise. Element k sits to_edge_k
    from its one near rounding boundary, on the side sign(ln - bf(ln)); it
    flips (by one bf16 spacing, that way) once eps (ln - beta) carries it
    there, i.e. for eps of one sign and |eps| >= to_edge / |ln - beta|. For
    each sign of eps the elements flip in order of that threshold, so the
    product moves by a prefix sum of signed terms sp_k B[k, n]: the term is
    the largest such prefix, over both signs. Elements within the
    evaluation noise of their boundary can flip either way on their own
    and are added by absolute value."""
    r = bf(ln)
    sp = bf16_spacing(ln)
    side = torch.sign(ln - r)
    to_edge = sp / 2 - (ln - r).abs()
    d = ln - beta
    noise = 16 * U * (d.abs() + beta.abs())
    loose = (to_edge <= noise).double()
    out = (loose * sp) @ B.abs()
    need = to_edge / d.abs().clamp_min(1e-300)
    for m in range(ln.shape[0]):
        best = torch.zeros_like(out[m])
        for sgn in (1.0, -1.0):
            k = torch.nonzero((need[m] <= LN_STATS_TOL) & (loose[m] == 0)
                              & (torch.sign(d[m]) * sgn == side[m]))[:, 0]
            if k.numel():
                k = k[torch.argsort(need[m, k])]
                steps = (side[m, k] * sp[m, k])[:, None] * B[k, :]
                best = torch.maximum(best, steps.cumsum(0).abs().amax(0))
        out[m] = out[m] + best
    return out


@functools.lru_cache(maxsize=None)
def ref2(c):
    return Ref2(c)


def _ratio(got, c, bound):
    r = ref2(c)
    assert got.shape == r.out.shape, (got.shape, r.out.shape)
    g = got.double()
    err = (g - r.out).abs()
    if c.out_dtype == BF16:
        # got = round-to-nearest of some v with |got - v| <= half the bf16
        # spacing at got: only the rest of the distance is v's own error
        err = (err - bf16_spacing(g) / 2).clamp_min(0)
    ratio = err / bound
    return float("inf") if torch.isnan(ratio).any() else ratio.max().item()


def check_bound(got, c):
    """worst err / bound of a layer-2 result of the output dtype (inf for
    a NaN)"""
    got = got.detach().cpu()
    assert got.dtype == c.out_dtype, (got.dtype, c.out_dtype)
    return _ratio(got, c, ref2(c).bound)


def honest_model(c):
    """fp32 torch on the CPU (host BLAS order), rounded only where the
    kernels round: the output, and the normalised row in the bf16 MFMA
    skinny form"""
    inp = inputs2(c)
    A = inp.A.float()
    if c.ln:
        mu = A.mean(-1, keepdim=True)
        d = A - mu
        inv = torch.rsqrt(d.pow(2).mean(-1, keepdim=True) + LN_EPS)
        A = d * inv * inp.gamma + inp.beta
        if c.mfma_skinny:
            A = bf(A)
    v = A @ inp.B.float()
    if c.has_ep:
        v = gelu_formula(v + inp.bias.float()) + inp.resid.float()
    return v.to(c.out_dtype)


def measure_a_act():
    """largest |gelu formula in fp32 - in float64| over the layer-2
    pre-activations (each taken as the fp32 value the kernel would hold)"""
    worst = 0.0
    for c in ALL_CASES:
        if 2 in c.layers and c.has_ep:
            p = ref2(c).pre.float()
            d = (gelu_formula(p).double() - gelu_formula(p.double())).abs()
            worst = max(worst, d.max().item())
    return worst


# name -> applies(case)
VARIANTS2 = {
    # two half-K slabs rounded to bf16 before the fold
    "slab_bf16": lambda c: c.R >= 2,
    # accumulator rounded to bf16 before the epilogue; a bf16 output rounds
    # the same value again and hides it
    "acc_bf16": lambda c: c.out_dtype == F32,
    "ln_no_beta": lambda c: c.ln,
    "ln_gamma_shift": lambda c: c.ln,
    # invstd changes by 1 / (2K) relative
    "ln_var_km1": lambda c: c.ln and c.dtype == F32,
}


def variant2_distance(c, name, issue=False):
    """err / bound of a wrong variant's result, rounded to the output dtype
    as a kernel would deliver it; issue=True measures plain |err| against
    the untightened bound"""
    v = Ref2(c, name).out
    if issue:
        r = ref2(c)
        return ((v - r.out).abs() / r.bound_issue).max().item()
    return _ratio(v.to(c.out_dtype), c, ref2(c).bound)
