"""Launches, float64 reference, rounding model and mutants for the extend
attention tests (test_attn_extend_oracle_cpu.py, test_gpu_attn_extend.py).

Extend attention gives, for T new query rows of a sequence whose cache
already holds P keys, rows P..P+T-1 of causal attention over S = P+T keys.
So every row of a launch is cut from an attn_oracle case: row b with prefix
P and T new tokens takes batch index b of attn_oracle.get_case(P+T, D, True);
its k, v fill cache slots [0, P+T), its q[P:] are the new queries, its
ref["o"][P:] is the float64 reference and emulate(...)["o"][P:] the rounding
model. Nothing here looks at a kernel's output.

Everything else in the launch's tensors is poison of full size: cache slots
>= P+T hold keys of the same distribution as real ones (randn*GAIN + bias*u)
and values 8*randn; query rows >= T of the shorter row are poisoned like the
keys. The one dead key right behind a row's last live key is, in addition,
moved along the row's last query until it would take half of that query's
softmax. A kernel that lets any of it in does not stay within the bound.

Metric: per (b, h), max|x - x64| / rms(x64) over the row's valid query rows;
a launch's error is the worst of them. The bound is attn_oracle.BOUND["o"],
unchanged.

extend64 is the rule itself in float64 on the launch's tensors (it must
reproduce the cut-out reference exactly), with the switches of the four
mutants: causal shift +1 / -1, every row using row 0's pos, and the keys of
the last ragged 64-key tile dropped.
"""

import functools
import math

import torch

import attn_oracle as A

B, H, CAP = A.B, A.H, 300
D_GRID = A.D_GRID
# (P, T) per row
LAUNCHES = [
    [(0, 1), (0, 17)],
    [(0, 64), (63, 1)],
    [(63, 2), (64, 1)],
    [(1, 64), (47, 17)],
    [(48, 17), (0, 129)],
    [(100, 100), (191, 9)],
    [(127, 130), (255, 2)],
    [(120, 8), (5, 3)],
    [(299, 1), (172, 128)],
]
CASES = [(i, D) for i in range(len(LAUNCHES)) for D in D_GRID]
VPOISON = 8.0


def case_id(case):
    i, D = case
    return "-".join(f"P{p}T{t}" for p, t in LAUNCHES[i]) + f"-D{D}"


@functools.lru_cache(maxsize=None)
def _model_o(S, D):
    c = A.get_case(S, D, True)
    return A.emulate(c.q, c.k, c.v, c.do, True)["o"]


def _key_like(shape, D, g):
    u = torch.full((D,), D ** -0.5)
    bias = math.sqrt(A.SHIFT * math.sqrt(D))
    return torch.randn(shape, generator=g) * A.GAIN + bias * u


class Launch:
    """tensors, reference and model error of one launch; built once per
    process and shared (treat as read-only)"""

    def __init__(self, idx, D):
        rows = LAUNCHES[idx]
        assert len(rows) == B
        self.idx, self.D, self.rows = idx, D, rows
        self.T = max(t for _, t in rows)
        g = torch.Generator().manual_seed(104729 * idx + D)
        q = _key_like((B, H, self.T, D), D, g)
        kc = _key_like((B, H, CAP, D), D, g)
        vc = torch.randn(B, H, CAP, D, generator=g) * VPOISON
        self.ref, self.model_o = [], []
        for b, (P, T) in enumerate(rows):
            c = A.get_case(P + T, D, True)
            q[b, :, :T] = c.q[b, :, P:].float()
            kc[b, :, :P + T] = c.k[b].float()
            vc[b, :, :P + T] = c.v[b].float()
            if P + T < CAP:
                # the dead slot right behind the last live key is moved
                # along the last query until it would take half of that
                # row's softmax if it were let in (what make_inputs does
                # with the spiked rows' own keys): a key visible one slot
                # too far cannot hide below the others by chance
                qr = c.q[b, :, -1].float()                       # [H, D]
                sc = D ** -0.5
                live = torch.einsum("hd,hjd->hj", qr, c.k[b].float()) * sc
                dead = (qr * kc[b, :, P + T]).sum(-1) * sc
                delta = torch.logsumexp(live, -1) - dead
                kc[b, :, P + T] += (delta / (qr.pow(2).sum(-1) * sc)
                                    )[:, None] * qr
            self.ref.append(c.ref["o"][b, :, P:])
            self.model_o.append(_model_o(P + T, D)[b, :, P:])
        self.q, self.kc, self.vc = (t.to(torch.bfloat16) for t in (q, kc, vc))
        self.pos = torch.tensor([p for p, _ in rows], dtype=torch.int64)
        self.n_new = torch.tensor([t for _, t in rows], dtype=torch.int64)
        self.model = self.error(self.model_o)

    def error(self, o):
        """worst nerr over the rows; o is [B,H,T,D] or a list of per-row
        [H,T_b,D] tensors"""
        return max(A.nerr(o[b][:, :T], self.ref[b])
                   for b, (_, T) in enumerate(self.rows))

    def dead_rows_zero(self, o):
        return all(bool((o[b][:, T:] == 0).all())
                   for b, (_, T) in enumerate(self.rows))

    def check(self, tag, o):
        """print kernel nerr next to the model's, then assert the bound"""
        e = self.error(o)
        print(f"{tag}: o kernel {e:.3e} model {self.model:.3e} "
              f"bound {A.BOUND['o']:.3e}")
        assert e <= A.BOUND["o"], f"{tag}: over the bound: {e}"
        return e

    def nan_poisoned(self):
        """(kc, vc) with NaN in K and V of every dead slot"""
        kc, vc = self.kc.clone(), self.vc.clone()
        for b, (P, T) in enumerate(self.rows):
            kc[b, :, P + T:] = float("nan")
            vc[b, :, P + T:] = float("nan")
        return kc, vc


@functools.lru_cache(maxsize=None)
def get_launch(idx, D):
    return Launch(idx, D)


def extend64(q, kc, vc, pos, n_new, *, causal_shift=0, row0_pos=False,
             drop_tail=False):
    """float64 extend attention on a launch's tensors: [B,H,T,D], rows
    >= n zero. All switches off: the rule."""
    q, kc, vc = (t.double() for t in (q, kc, vc))
    Bq, Hq, T, D = q.shape
    cap = kc.shape[2]
    o = torch.zeros(Bq, Hq, T, D, dtype=torch.float64)
    for b in range(Bq):
        p0 = int(pos[0 if row0_pos else b])
        p0 = min(max(p0, 0), cap)
        n = min(max(int(n_new[b]), 0), T, cap - p0)
        kv_len = p0 + n
        if n == 0:
            continue
        # for a live row the causal rule alone keeps every key below
        # kv_len, so a kernel whose rule is off by +1 reads the dead slot
        # behind the last live key: the mutant sees the cache as it is
        kv_len = min(kv_len + max(causal_shift, 0), cap)
        s = q[b, :, :n] @ kc[b, :, :kv_len].transpose(-1, -2) * D ** -0.5
        i = torch.arange(n)[:, None]
        j = torch.arange(kv_len)[None, :]
        s = s.masked_fill(j > p0 + i + causal_shift, float("-inf"))
        if drop_tail and kv_len % A.TILE:     # (shift and tail never mix)
            s[..., (kv_len // A.TILE) * A.TILE:] = float("-inf")
        lse = torch.logsumexp(s, dim=-1)
        p = torch.where(torch.isinf(lse)[..., None], torch.zeros_like(s),
                        torch.exp(s - lse[..., None]))
        o[b, :, :n] = p @ vc[b, :, :kv_len]
    return o


def _differ(idx, f):
    return any(f(*LAUNCHES[idx][b], b) for b in range(B))


# name -> (extend64 switches, applies(launch index): does it change the math
# of at least one row there)
MUTANTS = {
    "causal_sees_one_future_key": (
        dict(causal_shift=1), lambda i: True),
    "causal_hides_own_key": (
        dict(causal_shift=-1), lambda i: True),
    "every_row_uses_row0_pos": (
        dict(row0_pos=True),
        lambda i: LAUNCHES[i][1][0] != LAUNCHES[i][0][0]),   # not launch 0
    "drop_ragged_tail_keys": (
        dict(drop_tail=True),                                # not launch 1
        lambda i: _differ(i, lambda P, T, b: (P + T) % A.TILE != 0)),
}


def mutant_error(name, case):
    L = get_launch(*case)
    return L.error(extend64(L.q, L.kc, L.vc, L.pos, L.n_new,
                            **MUTANTS[name][0]))
