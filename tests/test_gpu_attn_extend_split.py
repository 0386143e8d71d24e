"""attn::k_attn_ext_split + k_attn_ext_fin on the GPU: the split-KV oracle's
launches (attn_extend_split_oracle.py; bound and teeth proven in
test_attn_extend_split_oracle_cpu.py) at every split count, dead rows and
dead cache slots, run-to-run bits, the merged-QKV layout, hipGraph capture
and the binding's new rejections."""

import functools
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_oracle as A  # noqa: E402
import attn_extend_split_oracle as X  # noqa: E402

if torch.cuda.is_available():
    from tnn_amd import _C
    ext = _C.ext()

from tnn_amd import ops  # noqa: E402

DEV = "cuda"


@functools.lru_cache(maxsize=None)
def _dev(idx, D):
    """the launch's tensors on the GPU, shared (read-only)"""
    L = X.get_launch(idx, D)
    kn, vn = L.nan_poisoned()
    merged = torch.randn(X.B, L.T, 3 * X.H * D,
                         generator=torch.Generator().manual_seed(5)) \
        .to(torch.bfloat16)
    # q takes the middle third: the base is offset as well as the strides
    merged[..., X.H * D:2 * X.H * D] = \
        L.q.transpose(1, 2).reshape(X.B, L.T, X.H * D)
    merged = merged.to(DEV)
    qv = merged[..., X.H * D:2 * X.H * D].view(X.B, L.T, X.H, D) \
        .transpose(1, 2)
    return dict(q=L.q.to(DEV), qv=qv, kc=L.kc.to(DEV), vc=L.vc.to(DEV),
                kn=kn.to(DEV), vn=vn.to(DEV), pos=L.pos.to(DEV),
                n_new=L.n_new.to(DEV))


def _run(t, ns, q="q", kc="kc", vc="vc"):
    return ext.attn_extend(t[q], t[kc], t[vc], t["pos"], t["n_new"],
                           t["q"].shape[-1] ** -0.5, ns)


@pytest.mark.parametrize("case", X.CASES, ids=X.case_id)
def test_oracle_launch(case):
    idx, D, ns = case
    L, t = X.get_launch(idx, D), _dev(idx, D)
    o = _run(t, ns)
    assert o.shape == L.q.shape and o.dtype == torch.bfloat16
    assert o.transpose(1, 2).is_contiguous()
    L.check(X.case_id(case), o.cpu(), ns)
    assert L.dead_rows_zero(o.cpu())
    # uninitialised workspaces, no atomics: a second call gives the same bits
    assert torch.equal(_run(t, ns), o)
    # NaN in every dead K and V slot changes no bit
    assert torch.isnan(t["kn"]).any() or all(
        P + T == X.CAP for P, T in L.rows)
    assert torch.equal(_run(t, ns, kc="kn", vc="vn"), o)
    # head slices of a merged [B,T,3*H*D] buffer against the dense q
    assert not t["qv"].is_contiguous() or L.T == 1
    assert torch.equal(t["qv"], t["q"])
    assert torch.equal(_run(t, ns, q="qv"), o)
    # the op passes the count through to the same kernel
    o2 = ops.attention_extend(t["q"], t["kc"], t["vc"], t["pos"], t["n_new"],
                              kv_splits=ns)
    assert torch.equal(o2, o)


@pytest.mark.parametrize("lcase", X.LCASES, ids=X.launch_id)
def test_kv_splits_zero_is_the_call_without_it(lcase):
    t = _dev(*lcase)
    scale = lcase[1] ** -0.5
    a = ext.attn_extend(t["q"], t["kc"], t["vc"], t["pos"], t["n_new"], scale)
    assert torch.equal(_run(t, 0), a)
    assert torch.equal(ext.attn_extend(t["q"], t["kc"], t["vc"], t["pos"],
                                       t["n_new"], scale, kv_splits=0), a)
    X.get_launch(*lcase).check("unsplit " + X.launch_id(lcase), a.cpu(), 1)


def test_uniform_chunk_form_and_clamps():
    """n_new absent means all T rows; pos past the cache or negative and
    n_new out of range are clamped in the kernel: no read outside the
    cache, rows past the clamp come back zero"""
    L, t = X.get_launch(3, 64), _dev(3, 64)
    full = torch.full((X.B,), L.T, dtype=torch.int64, device=DEV)
    pos = torch.tensor([150, 7], device=DEV)
    a = ext.attn_extend(t["q"], t["kc"], t["vc"], pos, None, 0.125, 4)
    b = ext.attn_extend(t["q"], t["kc"], t["vc"], pos, full, 0.125, 4)
    assert torch.equal(a, b)
    want = X.split64(L.q, L.kc, L.vc, pos.cpu(), full.cpu(), 4)
    assert A.nerr(a, want) <= A.BOUND["o"]
    for p, n in (([X.CAP + 5, X.CAP - 2], [3, 1 << 40]), ([-4, 0], [2, -1])):
        pos = torch.tensor(p, device=DEV)
        n_new = torch.tensor(n, device=DEV)
        want = X.split64(L.q, L.kc, L.vc, pos.cpu(), n_new.cpu(), 3)
        o = ext.attn_extend(t["q"], t["kc"], t["vc"], pos, n_new, 0.125,
                            3).cpu()
        assert bool((o[want == 0] == 0).all())
        for b_ in range(X.B):
            live = int((want[b_].abs().sum((0, 2)) > 0).sum())
            if live:
                assert A.nerr(o[b_, :, :live], want[b_, :, :live]) \
                    <= A.BOUND["o"]
        assert torch.isfinite(o.float()).all()


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("ns", [3, 16])
def test_graph_replay_follows_pos_and_n_new(D, ns):
    """captured with launch 4's rows, replayed with the two rows swapped:
    the grid is fixed by shapes, the split of the live range moves with
    pos / n_new on the device"""
    L, t = X.get_launch(4, D), _dev(4, D)
    st = {k: t[k].clone() for k in ("q", "kc", "vc", "pos", "n_new")}
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        _run(st, ns)                              # warm-up
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o_static = _run(st, ns)
    graph.replay()
    assert torch.equal(o_static, _run(t, ns))
    for k in st:
        st[k].copy_(t[k].flip(0))
    graph.replay()
    sw = {k: t[k].flip(0).contiguous() for k in st}
    o_eager = _run(sw, ns)
    assert torch.equal(o_static, o_eager)
    assert not torch.equal(o_static, _run(t, ns))
    L.check(f"swapped replay D{D} NS{ns}", o_static.flip(0).cpu(), ns)


def test_rejections():
    t = _dev(3, 64)
    _run(t, 16)                                   # the base arguments pass
    for ns in (-1, 17):
        with pytest.raises(RuntimeError):
            _run(t, ns)
        with pytest.raises(RuntimeError):
            ops.attention_extend(t["q"], t["kc"], t["vc"], t["pos"],
                                 t["n_new"], kv_splits=ns)
    q17 = torch.zeros(X.B, X.H, 17, 64, dtype=torch.bfloat16, device=DEV)
    n17 = torch.ones(X.B, dtype=torch.int64, device=DEV)
    ext.attn_extend(q17, t["kc"], t["vc"], t["pos"], n17, 0.125, 0)
    with pytest.raises(RuntimeError):
        ext.attn_extend(q17, t["kc"], t["vc"], t["pos"], n17, 0.125, 1)
    # today's checks still apply on the split route
    with pytest.raises(RuntimeError):
        ext.attn_extend(t["q"].float(), t["kc"], t["vc"], t["pos"],
                        t["n_new"], 0.125, 2)
    with pytest.raises(RuntimeError):
        ext.attn_extend(t["q"], t["kc"], t["vc"], t["pos"].int(),
                        t["n_new"], 0.125, 2)


def test_automatic_split_count_is_a_function_of_shapes():
    for BH in (1, 12, 64, 96, 160, 256, 4096):
        for cap in (16, 64, 65, 320, 1024, 4096):
            for T in (1, 5, 8, 16):
                ns = ext.attn_extend_splits(BH, cap, T)
                assert 0 <= ns <= min(16, -(-cap // 64)), (BH, cap, T, ns)
                assert ns == ext.attn_extend_splits(BH, cap, T)
            for T in (17, 64, 1000):
                assert ext.attn_extend_splits(BH, cap, T) == 0
