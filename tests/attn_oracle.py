"""Float64 oracle, rounding model, metric, inputs and mutants for the flash
attention tests (test_attn_oracle_cpu.py, test_gpu_attention_oracle.py).

Everything here is torch on the CPU. Nothing in this module looks at a
kernel's output: the bounds come from `emulate` (fp32, rounded only where
attention.hip rounds) measured against `ref64`, times FACTOR.

Metric
  o, dq, dk, dv:  nerr = max over (b, h) of max|x - x64| / rms(x64[b, h])
  lse:            max |lse - lse64|   (it is already a log)

Inputs (make_inputs)
  unit normals from a seeded CPU generator, B=2, H=3, then
  * q and k times GAIN=2: scaled scores get a standard deviation of 4, so a
    row's softmax sits on a handful of keys and each key matters;
  * every key gets +KBIAS along the unit vector u = 1/sqrt(D), and the query
    rows in spike_rows(S) get -QBIAS along u. A common offset on all of a
    row's scores leaves the softmax unchanged, but it drops those rows'
    scores to about -12, so a zero-padded key (score 0) that is let into the
    softmax takes the row over instead of hiding below e^10;
  * v and do rows in spike_rows(S) times SPIKE=2: the last key S-1 and the
    keys on both sides of the 64 and 128 tile edges carry values (and, on
    the query side, upstream gradients) that a dropped or doubled tile row
    cannot lose quietly;
  * k[r] of each spiked row r is moved along q[r] until row r gives its own
    key half of its softmax. Under causal masking key S-1 is seen by row
    S-1 alone, and with plain random inputs that one probability is as
    often 1e-6 as 0.5; this makes that one row count, and keeps dS = P (dP
    - Di) of the row away from the one-hot case where it vanishes.
  The query-side spike goes on do and not on q's magnitude: a larger q row
  sharpens that row's softmax to one-hot, and the row stops contributing
  to dK at all. SPIKE stays at 2 because the metric is max error over rms:
  a few rows 8 times larger raise the model's own dq floor from 0.12 to
  0.67 and bring the mutants no further from it.

Mutants (MUTANTS) are wrong variants of the float64 reference; see
test_attn_oracle_cpu.py for the separation they must keep from the bounds.
"""

import functools
import math

import torch

B, H = 2, 3
S_GRID = [1, 17, 63, 64, 65, 127, 128, 129, 191, 200, 257]
D_GRID = [64, 128]
CASES = [(S, D, c) for S in S_GRID for D in D_GRID for c in (False, True)]
KINDS = ("o", "lse", "dq", "dk", "dv")

GAIN = 2.0
SPIKE = 2.0
SHIFT = 12.0      # how far the spiked query rows' scores are pushed down
TILE = 64

# Worst nerr of the rounding model against float64 over CASES and over the
# spiked-K cases of the GPU file (measured on the CPU, asserted by
# test_attn_oracle_cpu.test_floor_is_what_the_bounds_were_set_from).
FLOOR = {"o": 2.52e-2, "lse": 1.50e-3, "dq": 1.173e-1, "dk": 9.87e-2,
         "dv": 3.60e-2}
FACTOR = 3.0      # __expf, MFMA summation order, dQ atomic order
BOUND = {k: FACTOR * f for k, f in FLOOR.items()}
TEETH = 3.0       # every mutant must reach TEETH * BOUND


def case_id(case):
    S, D, causal = case
    return f"S{S}-D{D}-{'causal' if causal else 'full'}"


def spike_rows(S):
    return sorted({r for r in (S - 1, 63, 64, 127, 128) if 0 <= r < S})


def make_inputs(S, D, causal, kspike=None):
    """bf16 q, k, v, do [B, H, S, D] on the CPU. kspike=(row, factor)
    multiplies one K row (the spiked-backward cases)."""
    g = torch.Generator().manual_seed(7919 * S + 2 * D + int(causal))
    q, k, v, do = (torch.randn(B, H, S, D, generator=g) for _ in range(4))
    u = torch.full((D,), D ** -0.5)
    bias = math.sqrt(SHIFT * math.sqrt(D))      # QBIAS = KBIAS
    rows = spike_rows(S)
    q, k = q * GAIN, k * GAIN + bias * u
    q[:, :, rows] -= bias * u
    v[:, :, rows] *= SPIKE
    do[:, :, rows] *= SPIKE
    # row r's own key gets half of row r's softmax: move k[r] along q[r]
    # until s[r, r] equals the logsumexp of the other keys that row r sees
    scale = D ** -0.5
    for r in rows:
        vis = [j for j in range(r if causal else S) if j != r]
        if not vis:
            continue
        qr = q[:, :, r]                                         # [B, H, D]
        s = torch.einsum("bhd,bhjd->bhj", qr, k) * scale
        delta = torch.logsumexp(s[..., vis], -1) - s[..., r]
        k[:, :, r] += (delta / (qr.pow(2).sum(-1) * scale))[..., None] * qr
    if kspike is not None:
        k[:, :, kspike[0]] *= kspike[1]
    return tuple(t.to(torch.bfloat16) for t in (q, k, v, do))


def rms(x):
    return x.double().pow(2).mean(dim=(-2, -1)).sqrt()


def nerr(x, x64, denom=None):
    """max over (b, h) of max|x - x64| / rms(x64[b, h]). `denom` replaces
    x64 in the denominator where x64 is identically zero (S=1 dq/dk)."""
    x = x.detach().double().cpu()
    d = (x - x64).abs().amax(dim=(-2, -1))
    r = rms(x64 if denom is None else denom)
    if not torch.isfinite(d).all():
        return float("inf")
    out = torch.where(d == 0, torch.zeros_like(d), d / r)
    return out.max().item()


def lse_err(x, x64):
    x = x.detach().double().cpu()
    e = (x - x64).abs()
    e = torch.where(x == x64, torch.zeros_like(e), e)   # -inf == -inf
    return float("inf") if torch.isnan(e).any() else e.max().item()


def _mask(S, Sk, causal, shift, dtype):
    """additive mask [S, Sk]: key j is visible to row i iff j <= i + shift"""
    m = torch.zeros(S, Sk, dtype=dtype)
    if causal:
        i = torch.arange(S)[:, None]
        j = torch.arange(Sk)[None, :]
        m = m.masked_fill(j > i + shift, float("-inf"))
    return m


def attn64(q, k, v, do, causal, *, drop_tail=False, pad_unmasked=False,
           causal_shift=0, other_scale=False, omit_di=False,
           dq_skip_last_kv_tile=False, dkv_skip_q_from=None):
    """float64 attention forward and backward in explicit form, with the
    switches the mutants flip. All switches off: the reference."""
    q, k, v, do = (t.double() for t in (q, k, v, do))
    S, D = q.shape[-2:]
    scale = (192 - D if other_scale else D) ** -0.5
    if pad_unmasked and S % TILE:
        pad = torch.zeros(*q.shape[:2], TILE - S % TILE, D, dtype=torch.float64)
        k, v = torch.cat([k, pad], 2), torch.cat([v, pad], 2)
    Sk = k.shape[-2]
    s = q @ k.transpose(-1, -2) * scale + _mask(S, Sk, causal, causal_shift,
                                                torch.float64)
    if drop_tail:
        s[..., (S // TILE) * TILE:] = float("-inf")
    lse = torch.logsumexp(s, dim=-1)
    # a row with no visible key: the kernel gives o = 0, lse = -inf
    p = torch.where(torch.isinf(lse)[..., None], torch.zeros_like(s),
                    torch.exp(s - lse[..., None]))
    o = p @ v
    di = torch.zeros_like(lse) if omit_di else (do * o).sum(-1)
    dp = do @ v.transpose(-1, -2)
    ds = p * (dp - di[..., None]) * scale
    nq = S if dkv_skip_q_from is None else dkv_skip_q_from
    dv = p[..., :nq, :].transpose(-1, -2) @ do[..., :nq, :]
    dk = ds[..., :nq, :].transpose(-1, -2) @ q[..., :nq, :]
    nk = ((S - 1) // TILE) * TILE if dq_skip_last_kv_tile else Sk
    dq = ds[..., :nk] @ k[..., :nk, :]
    return {"o": o, "lse": lse, "dq": dq, "dk": dk[..., :S, :],
            "dv": dv[..., :S, :]}


def ref64(q, k, v, causal):
    r = attn64(q, k, v, torch.zeros_like(q), causal)
    return r["o"], r["lse"]


def ref64_grads(q, k, v, do, causal):
    return attn64(q, k, v, do, causal)


def zero_ref_denoms(q, k, v, do, causal):
    """S=1: dq and dk are exactly zero because dP - Di cancels. The
    denominator for them is the float64 gradient with that cancellation
    removed (Di omitted), i.e. the size of the terms that cancel."""
    r = attn64(q, k, v, do, causal, omit_di=True)
    return {"dq": r["dq"], "dk": r["dk"]}


def bf(x):
    return x.to(torch.bfloat16).float()


def mm(a, b):
    """fp32 matmul as one correctly rounded fp32 result per element: the
    products are summed in float64, so the model does not depend on the
    host BLAS's summation order (the kernels' own order is one of the
    things FACTOR is for)."""
    return (a.double() @ b.double()).float()


def emulate(q, k, v, do, causal):
    """fp32 on the CPU, rounded to bf16 exactly where attention.hip rounds.

    Forward (k_attn_fwd): fp32 scores from the bf16 operands; per 64-key
    tile P = exp(s - m_running) is rounded to bf16 before both P@V and the
    row sum (the sum rides the same MFMA through a ones row); o_acc and l
    are rescaled in fp32; o = o_acc / l rounded to bf16; lse = m + log l.
    Backward (k_attn_dot, k_attn_bwd): Di from dO and the bf16 o in fp32;
    P^T = exp(s - lse) in fp32, rounded to bf16 for dV only; dS = P (dP -
    Di) scale from the fp32 P, rounded to bf16 for both dK and dQ; fp32
    accumulation; dq, dk, dv rounded to bf16.
    """
    qf, kf, vf, dof = (t.float() for t in (q, k, v, do))
    S, D = q.shape[-2:]
    scale = torch.tensor(D, dtype=torch.float32).rsqrt()
    s = mm(qf, kf.transpose(-1, -2)) * scale + _mask(S, S, causal, 0,
                                                    torch.float32)
    m = torch.full(q.shape[:3], float("-inf"))
    l = torch.zeros(q.shape[:3])
    acc = torch.zeros(q.shape)
    for t0 in range(0, S, TILE):
        st = s[..., t0:t0 + TILE]
        m_new = torch.maximum(m, st.amax(-1))   # key 0 is visible: finite
        a = torch.exp(m - m_new)
        p = bf(torch.exp(st - m_new[..., None]))
        acc = acc * a[..., None] + mm(p, vf[..., t0:t0 + TILE, :])
        l = l * a + p.double().sum(-1).float()
        m = m_new
    o = (acc / l[..., None]).to(torch.bfloat16)
    lse = m + torch.log(l)

    di = (dof.double() * o.double()).sum(-1).float()
    p = torch.exp(s - lse[..., None])
    dv = mm(bf(p).transpose(-1, -2), dof)
    dp = mm(dof, vf.transpose(-1, -2))
    ds = bf(p * (dp - di[..., None]) * scale)
    dk = mm(ds.transpose(-1, -2), qf)
    dq = mm(ds, kf)
    return {"o": o, "lse": lse, "dq": dq.to(torch.bfloat16),
            "dk": dk.to(torch.bfloat16), "dv": dv.to(torch.bfloat16)}


def errors(got, ref, denoms=None):
    """{kind: nerr} of a result dict (or any subset of KINDS) against ref"""
    denoms = denoms or {}
    return {kd: (lse_err(got[kd], ref[kd]) if kd == "lse"
                 else nerr(got[kd], ref[kd], denoms.get(kd)))
            for kd in KINDS if kd in got}


class Case:
    """inputs, float64 reference and rounding-model errors of one case;
    built once per process and shared (treat as read-only)"""

    def __init__(self, S, D, causal, kspike=None):
        self.S, self.D, self.causal = S, D, causal
        self.q, self.k, self.v, self.do = make_inputs(S, D, causal, kspike)
        self.ref = ref64_grads(self.q, self.k, self.v, self.do, causal)
        self.denoms = (zero_ref_denoms(self.q, self.k, self.v, self.do, causal)
                       if S == 1 else {})
        self.model = errors(emulate(self.q, self.k, self.v, self.do, causal),
                            self.ref, self.denoms)

    def errors(self, got):
        return errors(got, self.ref, self.denoms)

    def check(self, tag, got):
        """print kernel nerr next to the model's, then assert the bounds"""
        e = self.errors(got)
        print(f"{tag}: " + " | ".join(
            f"{kd} kernel {e[kd]:.3e} model {self.model[kd]:.3e} "
            f"bound {BOUND[kd]:.3e}" for kd in e))
        bad = {kd: x for kd, x in e.items() if not x <= BOUND[kd]}
        assert not bad, f"{tag}: over the bound: {bad}"
        return e


@functools.lru_cache(maxsize=None)
def get_case(S, D, causal, kspike=None):
    return Case(S, D, causal, kspike)


# spiked-backward cases of the GPU file: one K row of the last tile times 8
KSPIKE_CASES = [(200, D, True, (195, 8.0)) for D in D_GRID]


def _last_q_tile(S):
    return ((S - 1) // TILE) * TILE


# name -> (attn64 switches for a case, outputs it corrupts, applies(case),
#          cases skipped because the mutant is a mathematical no-op there)
MUTANTS = {
    "drop_ragged_tail_keys": (
        lambda S, D, c: dict(drop_tail=True), ("o",),
        lambda S, D, c: S % TILE != 0, ()),
    "padded_keys_unmasked": (
        lambda S, D, c: dict(pad_unmasked=True), ("o",),
        lambda S, D, c: S % TILE != 0 and not c, ()),
    "causal_sees_one_future_key": (
        lambda S, D, c: dict(causal_shift=1), ("o",),
        lambda S, D, c: c, (1,)),          # S=1 has no future key
    "causal_hides_own_key": (
        lambda S, D, c: dict(causal_shift=-1), ("o",),
        lambda S, D, c: c, ()),
    "scale_of_other_head_size": (
        lambda S, D, c: dict(other_scale=True), ("o",),
        lambda S, D, c: True, (1,)),       # softmax over one key is 1
    "di_omitted": (
        lambda S, D, c: dict(omit_di=True), ("dq", "dk"),
        lambda S, D, c: True, ()),
    "dq_misses_last_kv_tile": (
        lambda S, D, c: dict(dq_skip_last_kv_tile=True), ("dq",),
        lambda S, D, c: True, (1,)),       # dq is zero at S=1
    "dkdv_miss_last_q_tile": (
        lambda S, D, c: dict(dkv_skip_q_from=_last_q_tile(S)), ("dk", "dv"),
        lambda S, D, c: True, ()),
    "dkdv_miss_last_q_row": (
        lambda S, D, c: dict(dkv_skip_q_from=S - 1), ("dk", "dv"),
        lambda S, D, c: True, ()),
}
# outputs a mutant leaves exactly right at S=1 although it applies there
# (dk is zero at S=1 with or without the last q row)
NOOP_OUTPUTS = {("dkdv_miss_last_q_tile", 1): ("dk",),
                ("dkdv_miss_last_q_row", 1): ("dk",)}


def mutant_cases(name):
    _, _, applies, skip_s = MUTANTS[name]
    return [c for c in CASES if applies(*c) and c[0] not in skip_s]


def mutant_errors(name, case):
    """{output: nerr of the mutant against the reference} for the outputs
    the mutant corrupts on this case"""
    switches, outs, _, _ = MUTANTS[name]
    c = get_case(*case)
    got = attn64(c.q, c.k, c.v, c.do, c.causal, **switches(*case))
    outs = [o for o in outs if o not in NOOP_OUTPUTS.get((name, case[0]), ())]
    return errors({o: got[o] for o in outs}, c.ref, c.denoms)
