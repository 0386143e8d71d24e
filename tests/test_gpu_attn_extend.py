"""attn::k_attn_ext and k_kv_append_n on the GPU: the extend-attention
oracle's launches (attn_extend_oracle.py; bounds proven in
test_attn_extend_oracle_cpu.py), dead rows and dead cache slots, the
merged-QKV layout, binding rejections and hipGraph capture."""

import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_oracle as A  # noqa: E402
import attn_extend_oracle as X  # noqa: E402

if torch.cuda.is_available():
    from tnn_amd import _C
    ext = _C.ext()

from tnn_amd import ops  # noqa: E402

DEV = "cuda"


def _run(L, kc=None, vc=None, n_new=True, q=None):
    q = L.q.to(DEV) if q is None else q
    kc = (L.kc if kc is None else kc).to(DEV)
    vc = (L.vc if vc is None else vc).to(DEV)
    nn = L.n_new.to(DEV) if n_new else None
    return ext.attn_extend(q, kc, vc, L.pos.to(DEV), nn, L.D ** -0.5)


@pytest.mark.parametrize("case", X.CASES, ids=X.case_id)
def test_oracle_launch(case):
    L = X.get_launch(*case)
    o = _run(L)
    assert o.shape == L.q.shape and o.dtype == torch.bfloat16
    assert o.transpose(1, 2).is_contiguous()
    o = o.cpu()
    L.check(X.case_id(case), o)
    assert L.dead_rows_zero(o)
    # the op routes CUDA bf16 to the same kernel
    o2 = ops.attention_extend(L.q.to(DEV), L.kc.to(DEV), L.vc.to(DEV),
                              L.pos.to(DEV), L.n_new.to(DEV))
    assert torch.equal(o2.cpu(), o)


@pytest.mark.parametrize("case", [(5, 64), (6, 128)], ids=X.case_id)
def test_nan_in_dead_slots_changes_no_bit(case):
    L = X.get_launch(*case)
    kn, vn = L.nan_poisoned()
    assert torch.isnan(kn).any() and torch.isnan(vn).any()
    assert torch.equal(_run(L, kn, vn), _run(L))


@pytest.mark.parametrize("case", [(3, 64), (4, 128)], ids=X.case_id)
def test_merged_qkv_layout_is_bit_equal_to_dense(case):
    L = X.get_launch(*case)
    D, T = L.D, L.T
    g = torch.Generator().manual_seed(5)
    merged = torch.randn(X.B, T, 3 * X.H * D, generator=g).to(torch.bfloat16)
    # q takes the middle third: the base is offset as well as the strides
    merged[..., X.H * D:2 * X.H * D] = \
        L.q.transpose(1, 2).reshape(X.B, T, X.H * D)
    merged = merged.to(DEV)
    qv = merged[..., X.H * D:2 * X.H * D].view(X.B, T, X.H, D).transpose(1, 2)
    assert not qv.is_contiguous() and torch.equal(qv.cpu(), L.q)
    o = _run(L, q=qv)
    assert o.transpose(1, 2).is_contiguous()
    assert torch.equal(o, _run(L))


@pytest.mark.parametrize("T", [8, 17, 100])     # one size per wave count
def test_uniform_chunk_form(T):
    L = X.get_launch(8, 64)
    q = L.q[:, :, :T].contiguous().to(DEV)
    kc, vc = L.kc.to(DEV), L.vc.to(DEV)
    pos = torch.tensor([150, 7], device=DEV)
    full = torch.full((X.B,), T, dtype=torch.int64, device=DEV)
    a = ext.attn_extend(q, kc, vc, pos, None, 0.125)
    b = ext.attn_extend(q, kc, vc, pos, full, 0.125)
    assert torch.equal(a, b)
    want = X.extend64(q.cpu(), L.kc, L.vc, pos.cpu(), full.cpu())
    assert A.nerr(a, want) <= A.BOUND["o"]


def test_positions_are_clamped_in_the_kernel():
    """pos past the cache or negative, n_new out of range: no read outside
    the cache, rows past the clamp come back zero"""
    L = X.get_launch(7, 64)
    q, kc, vc = L.q.to(DEV), L.kc.to(DEV), L.vc.to(DEV)
    pos = torch.tensor([X.CAP + 5, X.CAP - 2], device=DEV)
    n_new = torch.tensor([3, 1 << 40], device=DEV)
    o = ext.attn_extend(q, kc, vc, pos, n_new, 0.125).cpu()
    assert bool((o[0] == 0).all()) and bool((o[1, :, 2:] == 0).all())
    want = X.extend64(L.q, L.kc, L.vc, pos.cpu(), n_new.cpu())
    assert A.nerr(o[1, :, :2], want[1, :, :2]) <= A.BOUND["o"]
    pos = torch.tensor([-4, 0], device=DEV)
    n_new = torch.tensor([2, -1], device=DEV)
    o = ext.attn_extend(q, kc, vc, pos, n_new, 0.125).cpu()
    want = X.extend64(L.q, L.kc, L.vc, pos.cpu(), n_new.cpu())
    assert A.nerr(o[0, :, :2], want[0, :, :2]) <= A.BOUND["o"]
    assert bool((o[0, :, 2:] == 0).all()) and bool((o[1] == 0).all())


# ---------------------------------------------------------------------------
# kv_append_n
# ---------------------------------------------------------------------------

def _kv_sources(Bn, Hn, T, D, dtype, seed=3):
    g = torch.Generator().manual_seed(seed)
    merged = torch.randn(Bn, T, 3 * Hn * D, generator=g).to(dtype).to(DEV)
    _, k, v = (t.view(Bn, T, Hn, D).transpose(1, 2)
               for t in merged.split(Hn * D, dim=-1))
    return k, v


# D=64 takes the 16-byte vector copy; D=20 rows are 40 bytes in bf16
# (element-wise) and 80 in fp32 (vectors)
@pytest.mark.parametrize("D", [64, 20])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_kv_append_n(dtype, D):
    Bn, Hn, T, cap = 3, 2, 5, 40
    k, v = _kv_sources(Bn, Hn, T, D, dtype)
    assert not k.is_contiguous()
    kc = torch.full((Bn, Hn, cap, D), 7.0, dtype=dtype, device=DEV)
    vc = torch.full((Bn, Hn, cap, D), -7.0, dtype=dtype, device=DEV)
    # the overflowing sequence comes first: a kernel that did not drop
    # rows 3 and 4 would write them into sequence 1's slots, not past the
    # tensor
    pos = torch.tensor([37, 0, 17], device=DEV)
    n_new = torch.tensor([5, 0, 3], device=DEV)
    ext.kv_append_n(kc, vc, k, v, pos, n_new)
    wk, wv = torch.full_like(kc, 7.0), torch.full_like(vc, -7.0)
    wk[0, :, 37:40], wv[0, :, 37:40] = k[0, :, :3], v[0, :, :3]
    wk[2, :, 17:20], wv[2, :, 17:20] = k[2, :, :3], v[2, :, :3]
    assert torch.equal(kc, wk) and torch.equal(vc, wv)
    # the op's torch form agrees
    ck = torch.full((Bn, Hn, cap, D), 7.0, dtype=dtype)
    cv = torch.full((Bn, Hn, cap, D), -7.0, dtype=dtype)
    ops.kv_append_n(ck, cv, k.cpu(), v.cpu(), pos.cpu(), n_new.cpu())
    assert torch.equal(ck, kc.cpu()) and torch.equal(cv, vc.cpu())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_kv_append_n_all_rows_and_negative_pos(dtype):
    Bn, Hn, T, D, cap = 3, 2, 5, 64, 40
    k, v = _kv_sources(Bn, Hn, T, D, dtype, seed=4)
    kc = torch.full((Bn, Hn, cap, D), 7.0, dtype=dtype, device=DEV)
    vc = torch.full((Bn, Hn, cap, D), -7.0, dtype=dtype, device=DEV)
    # the negative position sits on the last sequence: kept, its rows
    # would land inside sequence 1
    pos = torch.tensor([0, 33, -3], device=DEV)
    ops.kv_append_n(kc, vc, k, v, pos, None)
    wk, wv = torch.full_like(kc, 7.0), torch.full_like(vc, -7.0)
    wk[0, :, 0:5], wv[0, :, 0:5] = k[0], v[0]
    wk[1, :, 33:38], wv[1, :, 33:38] = k[1], v[1]
    assert torch.equal(kc, wk) and torch.equal(vc, wv)


# ---------------------------------------------------------------------------
# binding rejections: nothing is launched
# ---------------------------------------------------------------------------

def _ok_args(D=64, T=4, cap=16, Bn=2, Hn=2, dtype=torch.bfloat16):
    q = torch.zeros(Bn, Hn, T, D, dtype=dtype, device=DEV)
    kc = torch.zeros(Bn, Hn, cap, D, dtype=dtype, device=DEV)
    vc = torch.zeros_like(kc)
    pos = torch.zeros(Bn, dtype=torch.int64, device=DEV)
    n_new = torch.ones(Bn, dtype=torch.int64, device=DEV)
    return dict(q=q, kc=kc, vc=vc, pos=pos, n_new=n_new)


def _extend(a):
    return ext.attn_extend(a["q"], a["kc"], a["vc"], a["pos"], a["n_new"],
                           0.125)


def _append(a):
    return ext.kv_append_n(a["kc"], a["vc"], a["q"], a["q"], a["pos"],
                           a["n_new"])


def _misaligned_q(a):
    Bn, Hn, T, D = a["q"].shape
    return torch.zeros(Bn, Hn, T, D + 8, dtype=torch.bfloat16,
                       device=DEV)[..., 4:4 + D]


BOTH = {
    "q on the CPU": lambda a: a.update(q=a["q"].cpu()),
    "cache on the CPU": lambda a: a.update(kc=a["kc"].cpu()),
    "q of another dtype": lambda a: a.update(q=a["q"].float()),
    "caches disagree": lambda a: a.update(vc=a["vc"][:, :, :-1].contiguous()),
    "cache not contiguous": lambda a: a.update(
        kc=torch.zeros_like(a["kc"]).transpose(1, 2).contiguous()
        .transpose(1, 2)),
    "cache not 4-d": lambda a: a.update(kc=a["kc"][0], vc=a["vc"][0]),
    "q with another B": lambda a: a.update(q=a["q"][:1]),
    "q with another H": lambda a: a.update(q=a["q"][:, :1]),
    "q with another D": lambda a: a.update(
        q=torch.zeros(2, 2, 4, 128, dtype=torch.bfloat16, device=DEV)),
    "q d-stride not 1": lambda a: a.update(
        q=torch.zeros(2, 2, 64, 4, dtype=torch.bfloat16,
                      device=DEV).transpose(2, 3)),
    "T = 0": lambda a: a.update(q=a["q"][:, :, :0]),
    "T > cap": lambda a: a.update(
        q=torch.zeros(2, 2, 17, 64, dtype=torch.bfloat16, device=DEV)),
    "pos int32": lambda a: a.update(pos=a["pos"].int()),
    "pos on the CPU": lambda a: a.update(pos=a["pos"].cpu()),
    "pos of another length": lambda a: a.update(
        pos=torch.zeros(3, dtype=torch.int64, device=DEV)),
    "pos not contiguous": lambda a: a.update(
        pos=torch.zeros(4, dtype=torch.int64, device=DEV)[::2]),
    "n_new int32": lambda a: a.update(n_new=a["n_new"].int()),
    "n_new on the CPU": lambda a: a.update(n_new=a["n_new"].cpu()),
    "n_new not contiguous": lambda a: a.update(
        n_new=torch.zeros(4, dtype=torch.int64, device=DEV)[::2]),
}
EXTEND_ONLY = {
    "fp32": lambda a: a.update(_ok_args(dtype=torch.float32)),
    "D = 32": lambda a: a.update(_ok_args(D=32)),
    "rows not 16-byte aligned": lambda a: a.update(q=_misaligned_q(a)),
}


@pytest.mark.parametrize("what", list(BOTH) + list(EXTEND_ONLY))
def test_attn_extend_rejects(what):
    a = _ok_args()
    _extend(a)                                   # the base arguments pass
    {**BOTH, **EXTEND_ONLY}[what](a)
    with pytest.raises(RuntimeError):
        _extend(a)


@pytest.mark.parametrize("what", list(BOTH))
def test_kv_append_n_rejects(what):
    a = _ok_args()
    _append(a)
    BOTH[what](a)
    with pytest.raises(RuntimeError):
        _append(a)
    b = _ok_args()
    with pytest.raises(RuntimeError):            # k_new and v_new disagree
        ext.kv_append_n(b["kc"], b["vc"], b["q"], b["q"][:, :, :2], b["pos"],
                        None)


# ---------------------------------------------------------------------------
# hipGraph: fixed T, pos / n_new change between replays
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("D", [64, 128])
def test_graph_replay_follows_pos_and_n_new(D):
    Bn, Hn, T, cap = 3, 2, 8, 96
    g = torch.Generator().manual_seed(11)
    merged = torch.randn(Bn, T, 3 * Hn * D, generator=g) \
        .to(torch.bfloat16).to(DEV)
    q, k, v = (t.view(Bn, T, Hn, D).transpose(1, 2)
               for t in merged.split(Hn * D, dim=-1))
    kc0 = torch.randn(Bn, Hn, cap, D, generator=g).to(torch.bfloat16).to(DEV)
    vc0 = torch.randn(Bn, Hn, cap, D, generator=g).to(torch.bfloat16).to(DEV)
    kc, vc = kc0.clone(), vc0.clone()
    pos = torch.tensor([0, 5, 60], device=DEV)
    n_new = torch.tensor([8, 1, 3], device=DEV)
    scale = D ** -0.5

    def both(kc_, vc_):
        ext.kv_append_n(kc_, vc_, k, v, pos, n_new)
        return ext.attn_extend(q, kc_, vc_, pos, n_new, scale)

    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        both(kc, vc)                              # warm-up
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o_static = both(kc, vc)
    for p, n in (([64, 0, 88], [3, 8, 8]), ([7, 7, 7], [0, 8, 2])):
        pos.copy_(torch.tensor(p))
        n_new.copy_(torch.tensor(n))
        kc.copy_(kc0)
        vc.copy_(vc0)
        graph.replay()
        ke, ve = kc0.clone(), vc0.clone()
        o_eager = both(ke, ve)
        assert torch.equal(o_static, o_eager)
        assert torch.equal(kc, ke) and torch.equal(vc, ve)
        assert not torch.equal(kc, kc0)
