"""Launches, float64 split rule, rounding model and mutants for the split-KV
extend attention tests (test_attn_extend_split_oracle_cpu.py,
test_gpu_attn_extend_split.py).

Built like attn_extend_oracle.py: row b of a launch, with prefix P and T new
tokens, is batch index b of attn_oracle.get_case(P+T, D, True); its k, v
fill cache slots [0, P+T), its q[P:] are the new queries and its
ref["o"][P:] the float64 reference. Everything else is poison of full size
(key-like cache slots, 8*randn values, key-like dead query rows), and the
dead key right behind a row's last live key is moved along the row's last
query until it would take half of that query's softmax. Same metric, and
the unchanged bound attn_oracle.BOUND["o"]. Nothing here looks at a kernel's
output.

The kernel under test serves 1 <= T <= 16 and divides the LIVE KV tiles of a
row among NS blocks: ntiles = ceil((P+T) / 64), per = ceil(ntiles / NS),
split s walks tiles [s*per, min((s+1)*per, ntiles)). CAP = 640 is ten tiles;
with SPLITS = {1, 2, 3, 4, 8, 16} every launch meets uneven shares (ten
tiles over 3 and over 4), empty splits, and a one-tile row next to a
ten-tile row. Launch 6's first row has n_new == 0.

split64 is that rule in float64 on the launch's tensors: per-split
unnormalised (m, l, acc), folded in index order with weights exp(m_s - m).
Its switches are the mutants. emulate_split is the rounding model:
attn_oracle.emulate's roundings inside each split (P to bf16 before P@V and
the row sum, fp32 rescales), then the fp32 combine and one rounding of o.
"""

import functools

import torch

import attn_oracle as A
from attn_extend_oracle import VPOISON, _key_like

B, H, CAP = A.B, A.H, 640
D_GRID = A.D_GRID
TILE = A.TILE
TMAX = 16
# (P, T) per row
LAUNCHES = [
    [(0, 1), (0, 16)],
    [(63, 1), (64, 1)],
    [(127, 2), (128, 16)],
    [(300, 8), (5, 3)],
    [(191, 9), (255, 2)],
    [(624, 16), (639, 1)],
    [(100, 0), (200, 5)],
]
SPLITS = [1, 2, 3, 4, 8, 16]
LCASES = [(i, D) for i in range(len(LAUNCHES)) for D in D_GRID]
CASES = [(i, D, ns) for i, D in LCASES for ns in SPLITS]


def launch_id(lcase):
    i, D = lcase
    return "-".join(f"P{p}T{t}" for p, t in LAUNCHES[i]) + f"-D{D}"


def case_id(case):
    return launch_id(case[:2]) + f"-NS{case[2]}"


def split_tiles(kv_len, ns, s):
    """[t0, t1) of split s over a live length kv_len"""
    ntiles = -(-kv_len // TILE)
    per = -(-ntiles // ns)
    return s * per, min((s + 1) * per, ntiles)


class Launch:
    """tensors and reference of one launch; built once per process and
    shared (treat as read-only)"""

    def __init__(self, idx, D):
        rows = LAUNCHES[idx]
        assert len(rows) == B and all(0 <= t <= TMAX for _, t in rows)
        self.idx, self.D, self.rows = idx, D, rows
        self.T = max(t for _, t in rows)
        g = torch.Generator().manual_seed(15485863 * idx + D)
        q = _key_like((B, H, self.T, D), D, g)
        kc = _key_like((B, H, CAP, D), D, g)
        vc = torch.randn(B, H, CAP, D, generator=g) * VPOISON
        self.ref = []
        for b, (P, T) in enumerate(rows):
            if T == 0:          # a prefix the launch must not look at
                self.ref.append(torch.zeros(H, 0, D, dtype=torch.float64))
                continue
            c = A.get_case(P + T, D, True)
            q[b, :, :T] = c.q[b, :, P:].float()
            kc[b, :, :P + T] = c.k[b].float()
            vc[b, :, :P + T] = c.v[b].float()
            if P + T < CAP:
                # the spiked dead key behind the last live key, as in
                # attn_extend_oracle.Launch
                qr = c.q[b, :, -1].float()                       # [H, D]
                sc = D ** -0.5
                live = torch.einsum("hd,hjd->hj", qr, c.k[b].float()) * sc
                dead = (qr * kc[b, :, P + T]).sum(-1) * sc
                delta = torch.logsumexp(live, -1) - dead
                kc[b, :, P + T] += (delta / (qr.pow(2).sum(-1) * sc)
                                    )[:, None] * qr
            self.ref.append(c.ref["o"][b, :, P:])
        self.q, self.kc, self.vc = (t.to(torch.bfloat16) for t in (q, kc, vc))
        self.pos = torch.tensor([p for p, _ in rows], dtype=torch.int64)
        self.n_new = torch.tensor([t for _, t in rows], dtype=torch.int64)

    def error(self, o):
        """worst nerr over the live rows of o [B,H,T,D]"""
        return max(A.nerr(o[b][:, :T], self.ref[b])
                   for b, (_, T) in enumerate(self.rows) if T > 0)

    def dead_rows_zero(self, o):
        return all(bool((o[b][:, T:] == 0).all())
                   for b, (_, T) in enumerate(self.rows))

    def model(self, ns):
        return model_error(self.idx, self.D, ns)

    def check(self, tag, o, ns):
        """print kernel nerr next to the model's, then assert the bound"""
        e = self.error(o)
        print(f"{tag}: o kernel {e:.3e} model {self.model(ns):.3e} "
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


def _fold(parts, weights=True):
    """(m, l, acc) per split, in index order -> o; l_s == 0 is skipped"""
    m = torch.stack([p[0] for p in parts]).amax(0)
    l = torch.zeros_like(m)
    o = torch.zeros_like(parts[0][2])
    for ms, ls, acc in parts:
        w = torch.exp(ms - m) if weights else torch.ones_like(ms)
        w = torch.where(ls > 0, w, torch.zeros_like(w))
        l = l + ls * w
        o = o + acc * w[..., None]
    return torch.where(l[..., None] > 0, o / l[..., None], torch.zeros_like(o))


def split64(q, kc, vc, pos, n_new, ns, *, causal_shift=0, row0_pos=False,
            drop_last_split=False, no_weights=False, late=False,
            early=False):
    """float64 split-KV extend attention on a launch's tensors: [B,H,T,D],
    rows >= n zero. All switches off: the rule."""
    q, kc, vc = (t.double() for t in (q, kc, vc))
    Bq, Hq, T, D = q.shape
    cap = kc.shape[2]
    o = torch.zeros(Bq, Hq, T, D, dtype=torch.float64)
    for b in range(Bq):
        p0 = min(max(int(pos[0 if row0_pos else b]), 0), cap)
        n = min(max(int(n_new[b]), 0), T, cap - p0)
        kv_len = p0 + n
        if n == 0:
            continue
        # as in attn_extend_oracle.extend64: a rule off by +1 reaches the
        # dead slot behind the last live key, so that mutant sees the
        # cache as it is
        seen = min(kv_len + max(causal_shift, 0), cap)
        s_all = q[b, :, :n] @ kc[b, :, :seen].transpose(-1, -2) * D ** -0.5
        i = torch.arange(n)[:, None]
        j = torch.arange(seen)[None, :]
        s_all = s_all.masked_fill(j > p0 + i + causal_shift, float("-inf"))
        ntiles = -(-kv_len // TILE)
        spans = [split_tiles(kv_len, ns, s) for s in range(ns)]
        spans = [(t0, t1) for t0, t1 in spans if t0 < t1]
        if late:      # every later split starts one tile late
            spans = [(t0 + (k > 0), t1) for k, (t0, t1) in enumerate(spans)]
        if early:     # every split but the last runs one tile into the next
            spans = [(t0, min(t1 + 1, ntiles)) if k + 1 < len(spans)
                     else (t0, t1) for k, (t0, t1) in enumerate(spans)]
        if drop_last_split:
            spans = spans[:-1]
        parts = []
        for t0, t1 in spans:
            lo, hi = t0 * TILE, seen if t1 == ntiles else t1 * TILE
            st = s_all[..., lo:hi]
            ms = st.amax(-1) if hi > lo else torch.full(
                s_all.shape[:2], float("-inf"), dtype=torch.float64)
            p = torch.where(torch.isinf(st), torch.zeros_like(st),
                            torch.exp(st - ms[..., None]))
            parts.append((ms, p.sum(-1), p @ vc[b, :, lo:hi]))
        if parts:
            o[b, :, :n] = _fold(parts, weights=not no_weights)
    return o


def emulate_split(q, kc, vc, pos, n_new, ns):
    """The rounding model: fp32, rounded to bf16 where k_attn_ext_split
    rounds (attn_oracle.emulate's roundings within each split), then the
    fp32 combine of k_attn_ext_fin and one rounding of o."""
    qf, kf, vf = (t.float() for t in (q, kc, vc))
    Bq, Hq, T, D = q.shape
    scale = torch.tensor(D, dtype=torch.float32).rsqrt()
    o = torch.zeros(Bq, Hq, T, D, dtype=torch.bfloat16)
    for b in range(Bq):
        p0, n = int(pos[b]), int(n_new[b])
        kv_len = p0 + n
        if n == 0:
            continue
        s_all = A.mm(qf[b, :, :n], kf[b, :, :kv_len].transpose(-1, -2)) * scale
        i = torch.arange(n)[:, None]
        j = torch.arange(kv_len)[None, :]
        s_all = s_all.masked_fill(j > p0 + i, float("-inf"))
        parts = []
        for s in range(ns):
            t0, t1 = split_tiles(kv_len, ns, s)
            if t0 >= t1:
                continue
            m = torch.full((Hq, n), float("-inf"))
            l = torch.zeros(Hq, n)
            acc = torch.zeros(Hq, n, D)
            for t in range(t0, t1):
                st = s_all[..., t * TILE:(t + 1) * TILE]
                m_new = torch.maximum(m, st.amax(-1))
                dead = torch.isinf(m_new)        # no key seen so far
                a = torch.where(torch.isinf(m), torch.zeros_like(m),
                                torch.exp(m - m_new))
                a = torch.where(dead, torch.ones_like(a), a)
                p = A.bf(torch.where(torch.isinf(st), torch.zeros_like(st),
                                     torch.exp(st - m_new[..., None])))
                acc = acc * a[..., None] + A.mm(
                    p, vf[b, :, t * TILE:t * TILE + st.shape[-1]])
                l = l * a + p.double().sum(-1).float()
                m = m_new
            parts.append((m, l, acc))
        o[b, :, :n] = _fold(parts).to(torch.bfloat16)
    return o


@functools.lru_cache(maxsize=None)
def model_error(idx, D, ns):
    L = get_launch(idx, D)
    return L.error(emulate_split(L.q, L.kc, L.vc, L.pos, L.n_new, ns))


def _rows(idx):
    return [(P, T) for P, T in LAUNCHES[idx] if T > 0]


def _nonempty(P, T, ns):
    return sum(1 for s in range(ns)
               if split_tiles(P + T, ns, s)[0] < split_tiles(P + T, ns, s)[1])


def _two_splits(idx, ns):
    """some live row is shared by at least two non-empty splits"""
    return any(_nonempty(P, T, ns) >= 2 for P, T in _rows(idx))


# name -> (split64 switches, applies(launch index, ns): does it change the
# math of at least one live row there)
MUTANTS = {
    "last_nonempty_split_dropped": (
        dict(drop_last_split=True), lambda i, ns: True),
    "combine_without_weights": (
        dict(no_weights=True), _two_splits),
    "boundary_one_tile_late": (
        dict(late=True), _two_splits),
    "boundary_one_tile_early": (
        dict(early=True), _two_splits),
    "every_row_uses_row0_pos": (
        dict(row0_pos=True),
        lambda i, ns: LAUNCHES[i][1][0] != LAUNCHES[i][0][0]),  # not launch 0
    # caught through the spiked dead key behind a row's last live key; in
    # launch 5 both rows end at CAP and no such slot exists (there the rule
    # only shows rows 0..14 one more live key, a matter of chance)
    "causal_sees_one_future_key": (
        dict(causal_shift=1),
        lambda i, ns: any(P + T < CAP for P, T in _rows(i))),
    "causal_hides_own_key": (
        dict(causal_shift=-1), lambda i, ns: True),
}


def mutant_error(name, case):
    idx, D, ns = case
    L = get_launch(idx, D)
    return L.error(split64(L.q, L.kc, L.vc, L.pos, L.n_new, ns,
                           **MUTANTS[name][0]))
