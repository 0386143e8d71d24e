"""Batched GPU-resident decode: skinny GEMM (2 <= M <= 16), per-sequence
positions in decode attention, fused KV append, on-device sampling, and
generate_batch end to end (ragged prompts, hipGraph vs eager)."""

import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from tnn_amd import _C
    ext = _C.ext()

from tnn_amd import ops
from tnn_amd.ops.functional import ACT_KINDS, _sample_rules

DEV = "cuda"


def maxerr(a, b):
    return (a.float() - b.float()).abs().max().item()


def tol(dtype, K):
    return 3e-6 * K if dtype == torch.float32 else 2e-2 * (K ** 0.5)


# ---------------------------------------------------------------------------
# skinny GEMM: K-split, N % 64 != 0, ragged both ways; odd N takes the
# element-wise column mapping, even N the paired loads
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("KN", [(768, 768), (3072, 768), (768, 1000),
                                (100, 65)])
@pytest.mark.parametrize("M", [2, 3, 8, 16])
def test_gemm_skinny(M, KN, dtype):
    torch.manual_seed(9)
    K, N = KN
    x = torch.randn(M, K, dtype=dtype, device=DEV)
    w = torch.randn(K, N, dtype=dtype, device=DEV) * 0.05
    b = torch.randn(N, dtype=dtype, device=DEV)
    r = torch.randn(M, N, dtype=dtype, device=DEV)
    g = torch.rand(K, device=DEV) + 0.5
    be = torch.randn(K, device=DEV) * 0.1
    t = tol(dtype, K)
    xf, wf = x.float(), w.float()
    # bias only
    y = ext.gemm_skinny(x, w, b, ACT_KINDS["linear"])
    assert y.dtype == dtype and y.shape == (M, N)
    assert maxerr(y, xf @ wf + b.float()) < t
    # no bias at all
    assert maxerr(ext.gemm_skinny(x, w, None, ACT_KINDS["linear"]),
                  xf @ wf) < t
    # bias + gelu + residual
    y = ext.gemm_skinny(x, w, b, ACT_KINDS["gelu"], r)
    ref = torch.nn.functional.gelu(xf @ wf + b.float(),
                                   approximate="tanh") + r.float()
    assert maxerr(y, ref) < t
    # LayerNorm fused into the staging
    y = ext.gemm_skinny(x, w, b, ACT_KINDS["linear"], None, g, be, 1e-5)
    ln = torch.nn.functional.layer_norm(xf, (K,), g, be, 1e-5)
    assert maxerr(y, ln @ wf + b.float()) < t


def test_gemm_skinny_rejects_wide_m_and_dtypes():
    w = torch.randn(64, 64, device=DEV)
    with pytest.raises(RuntimeError):
        ext.gemm_skinny(torch.randn(17, 64, device=DEV), w, None, 0)
    with pytest.raises(RuntimeError):
        ext.gemm_skinny(torch.randn(4, 64, device=DEV).half(), w.half(),
                        None, 0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_linear_routes_small_batches_through_skinny(dtype):
    torch.manual_seed(1)
    K, N = 256, 192
    x = torch.randn(2, 2, K, dtype=dtype, device=DEV)   # M = 4 rows
    w = torch.randn(K, N, dtype=dtype, device=DEV) * 0.05
    b = torch.randn(N, dtype=dtype, device=DEV)
    g = torch.rand(K, device=DEV) + 0.5
    be = torch.randn(K, device=DEV) * 0.1
    x2 = x.reshape(-1, K).contiguous()
    with torch.no_grad():
        y = ops.linear(x, w, b, act="gelu", residual=None, ln=(g, be, 1e-5))
    want = ext.gemm_skinny(x2, w, b, ACT_KINDS["gelu"], None, g, be, 1e-5)
    assert y.shape == (2, 2, N)
    assert torch.equal(y.reshape(-1, N), want)


def skinny_off_check():
    """Run by the child of the test below, under TNN_SKINNY=0: linear must
    give exactly what the general path (ext.gemm) gives."""
    torch.manual_seed(1)
    x = torch.randn(4, 256, dtype=torch.bfloat16, device=DEV)
    w = torch.randn(256, 192, dtype=torch.bfloat16, device=DEV) * 0.05
    b = torch.randn(192, dtype=torch.bfloat16, device=DEV)
    with torch.no_grad():
        y = ops.linear(x, w, b, act="gelu")
    return (not ext.skinny_enabled()
            and torch.equal(y, ext.gemm(x, w, b, ACT_KINDS["gelu"])))


def test_skinny_kill_switch_fresh_process():
    # the switch is read once per process, so it needs a process of its own
    import os, subprocess, sys
    assert ext.skinny_enabled()
    here = os.path.dirname(os.path.abspath(__file__))
    child = ("import sys; sys.path[:0] = [%r, %r]; "
             "import test_gpu_decode_batch as t; "
             "print('SKINNY_OFF', t.skinny_off_check())"
             % (os.path.dirname(here), here))
    r = subprocess.run([sys.executable, "-c", child],
                       env=dict(os.environ, TNN_SKINNY="0"),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "SKINNY_OFF True" in r.stdout, r.stdout[-500:]


# ---------------------------------------------------------------------------
# attn_decode with one position per sequence; fused KV append
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("D", [64, 128])
def test_attn_decode_per_sequence_positions(D):
    torch.manual_seed(6)
    B, H, cap = 3, 2, 300
    pos_l = [0, 255, 299]   # length 1, the 256-wide tile edge, full
    q = torch.randn(B * H, D, dtype=torch.bfloat16, device=DEV)
    k = torch.randn(B * H, cap, D, dtype=torch.bfloat16, device=DEV)
    v = torch.randn(B * H, cap, D, dtype=torch.bfloat16, device=DEV)
    scale = D ** -0.5
    pos = torch.tensor(pos_l, dtype=torch.int64, device=DEV)
    o = ext.attn_decode(q, k, v, pos, 0, scale)
    for b, p in enumerate(pos_l):
        sl = slice(b * H, (b + 1) * H)
        n = p + 1
        # same split count (16) on both sides at these sizes: bit-equal
        one = ext.attn_decode(q[sl].contiguous(), k[sl].contiguous(),
                              v[sl].contiguous(), None, n, scale)
        assert torch.equal(o[sl], one), (b, p)
        s = (q[sl].float().unsqueeze(1)
             @ k[sl, :n].float().transpose(-1, -2)) * scale
        ref = (torch.softmax(s, dim=-1) @ v[sl, :n].float()).squeeze(1)
        assert maxerr(o[sl], ref) < 3e-2
    with pytest.raises(RuntimeError):
        ext.attn_decode(q, k, v, pos[:2].repeat(2), 0, scale)   # 6 % 4 != 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_kv_append_touches_only_addressed_rows(dtype):
    torch.manual_seed(2)
    B, H, cap, D = 3, 2, 40, 64
    kc = torch.full((B, H, cap, D), 7.0, dtype=dtype, device=DEV)
    vc = torch.full((B, H, cap, D), -3.0, dtype=dtype, device=DEV)
    # the strided views _project hands over: slices of one [B, 1, 3*H*D] row
    qkv = torch.randn(B, 1, 3 * H * D, dtype=dtype, device=DEV)
    _, kn, vn = (t.view(B, 1, H, D).transpose(1, 2)
                 for t in qkv.split(H * D, dim=-1))
    assert not kn.is_contiguous()
    pos_l = [0, 17, 39]
    pos = torch.tensor(pos_l, dtype=torch.int64, device=DEV)
    ops.kv_append(kc, vc, kn, vn, pos)
    hit = torch.zeros(B, H, cap, dtype=torch.bool, device=DEV)
    for b, p in enumerate(pos_l):
        hit[b, :, p] = True
        assert torch.equal(kc[b, :, p], kn[b, :, 0])
        assert torch.equal(vc[b, :, p], vn[b, :, 0])
    assert torch.all(kc[~hit] == 7.0) and torch.all(vc[~hit] == -3.0)


# ---------------------------------------------------------------------------
# on-device sampling against the float64 torch form of the same rules
# ---------------------------------------------------------------------------

U_VALUES = [2.0 ** -24, 0.25, 0.5, 0.999, 1.0]


def _step(v=0):
    return torch.full((1,), v, dtype=torch.int64, device=DEV)


@pytest.fixture(scope="module", params=[50257, 257])
def logit_rows(request):
    V = request.param
    g = torch.Generator().manual_seed(V)
    base = (torch.randn(2, V, generator=g) * 2).to(torch.bfloat16)
    # every u against both rows
    rows = base.repeat_interleave(len(U_VALUES), dim=0).to(DEV)
    u = torch.tensor(U_VALUES * 2, dtype=torch.float32, device=DEV)
    return rows, u


@pytest.mark.parametrize("top_k,top_p", [(0, 1.0), (50, 1.0), (0, 0.9),
                                         (40, 0.95)])
def test_sample_explicit_u_matches_oracle_cdf(logit_rows, top_k, top_p):
    rows, u = logit_rows
    ids = ext.sample_logits(rows, 0.8, top_k, top_p, 0, _step(), u)
    assert ids.dtype == torch.int64 and ids.shape == (rows.shape[0],)
    keep, w = _sample_rules(rows, 0.8, top_k, top_p)
    cdf = (w / w.sum(-1, keepdim=True)).cumsum(-1)
    for r, i in enumerate(ids.tolist()):
        assert 0 <= i < rows.shape[1]
        assert keep[r, i], (r, i)
        lo = cdf[r, i - 1].item() if i > 0 else 0.0
        hi = cdf[r, i].item()
        ur = float(u[r].double())
        print(f"row {r} u={ur:.8f} id={i} cdf=({lo:.8f}, {hi:.8f}]")
        assert lo - 1e-4 <= ur <= hi + 1e-4, (r, i, lo, ur, hi)


def test_sample_greedy_modes(logit_rows):
    rows, _ = logit_rows
    rows = rows.clone()
    V = rows.shape[1]
    peak = torch.arange(rows.shape[0], device=DEV) * 13 % V
    rows[torch.arange(rows.shape[0], device=DEV), peak] = 30.0  # unique max
    for kw in (dict(temperature=0.8, top_k=1), dict(temperature=0.0, top_k=0),
               dict(temperature=0.0, top_k=5)):
        ids = ext.sample_logits(rows, kw["temperature"], kw["top_k"], 0.9, 3,
                                _step(2))
        assert torch.equal(ids, rows.float().argmax(-1))
        assert torch.equal(ids, peak)
    # a tie at the maximum returns the lowest index
    tie = rows[:1].clone()
    tie[0, V - 1] = 30.0
    tie[0, 5] = 30.0
    tie[0, int(peak[0])] = 0.0
    assert ext.sample_logits(tie, 0.0, 0, 1.0, 0, _step()).tolist() == [5]
    assert ext.sample_logits(tie, 1.0, 1, 1.0, 0, _step()).tolist() == [5]
    # ops wrapper takes the same kernel for bf16 GPU logits
    assert ops.sample_logits(tie, 0.0).tolist() == [5]


def _dominant_row():
    g = torch.Generator().manual_seed(4)
    row = torch.randn(1000, generator=g)
    hot = torch.randperm(1000, generator=g)[:10]
    row[hot] = torch.linspace(5.0, 8.0, 10)
    return row.to(torch.bfloat16).to(DEV)


def test_sample_philox_frequencies():
    R = 4096
    row = _dominant_row()
    rows = row.expand(R, -1).contiguous()
    ids = ext.sample_logits(rows, 1.0, 50, 0.99, 1234, _step(7))
    keep, w = _sample_rules(row[None], 1.0, 50, 0.99)
    assert torch.all(keep[0][ids])
    p = (w / w.sum())[0]
    freq = torch.bincount(ids, minlength=1000).double() / R
    checked = 0
    for t in (p >= 0.01).nonzero().flatten().tolist():
        pt = p[t].item()
        bound = 5 * (pt * (1 - pt) / R) ** 0.5
        print(f"token {t}: p={pt:.4f} freq={freq[t].item():.4f} "
              f"bound={bound:.4f}")
        assert abs(freq[t].item() - pt) <= bound, (t, pt, freq[t].item())
        checked += 1
    assert checked >= 5


def test_sample_is_a_function_of_seed_and_step():
    rows = _dominant_row().expand(4096, -1).contiguous()
    a = ext.sample_logits(rows, 1.0, 0, 1.0, 11, _step(3))
    assert torch.equal(a, ext.sample_logits(rows, 1.0, 0, 1.0, 11, _step(3)))
    assert not torch.equal(a, ext.sample_logits(rows, 1.0, 0, 1.0, 11,
                                                _step(4)))
    assert not torch.equal(a, ext.sample_logits(rows, 1.0, 0, 1.0, 12,
                                                _step(3)))


# ---------------------------------------------------------------------------
# end to end: dim 128 / 2 heads (D = 64, so the HIP decode kernels run),
# one flash and one materialized block, ragged prompts
# ---------------------------------------------------------------------------

SEQ, VOCAB = 64, 300
PROMPT_LENS = (1, 5, 12)


def _tiny(dtype):
    from tnn_amd.nn import LayerBuilder
    from tnn_amd.nn.layer import cast_compute_dtype
    torch.manual_seed(3)
    m = (LayerBuilder((SEQ,))
         .embedding(VOCAB, 128, "tok")
         .positional_embedding(SEQ, "pos")
         .gpt_block(2, 4, flash=True, name="b0")
         .gpt_block(2, 4, flash=False, name="b1")
         .layernorm(name="ln_f")
         .dense(VOCAB, True, "head")
         .build("tiny_gpt"))
    if dtype != torch.float32:
        cast_compute_dtype(m, dtype)
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def bf16_model():
    return _tiny(torch.bfloat16)


def _prompts(lens=PROMPT_LENS):
    g = torch.Generator().manual_seed(8)
    return [torch.randint(0, VOCAB, (n,), generator=g).tolist() for n in lens]


def test_batched_decoder_teacher_forced_logits(bf16_model):
    """Batched logits vs a CPU fp32 full recompute, with the B=1
    static-cache path (the parent's behaviour) on the same sequences as
    the yardstick: err_batched <= 2 * err_b1 + 1e-2 at every step."""
    from tnn_amd.models.generate import BatchedDecoder
    from tnn_amd.nn.layer import cast_compute_dtype
    steps = 6
    prompts = _prompts()
    g = torch.Generator().manual_seed(21)
    forced = torch.randint(0, VOCAB, (len(prompts), steps), generator=g)
    ref_m = copy.deepcopy(bf16_model).cpu().float()
    cast_compute_dtype(ref_m, torch.float32)
    refs = []   # refs[b][j]: logits after the prompt plus j forced tokens
    with torch.no_grad():
        for b, p in enumerate(prompts):
            full = torch.tensor([p + forced[b].tolist()])
            refs.append(ref_m(full)[0, len(p) - 1:].float())

    def run(rows):
        dec = BatchedDecoder(bf16_model, SEQ)
        try:
            out = [dec.prefill([prompts[b] for b in rows]).float().cpu()]
            for j in range(steps):
                out.append(dec.step(forced[rows, j]).float().cpu())
            return torch.stack(out, 1)          # [rows, steps + 1, V]
        finally:
            dec.close()

    batched = run([0, 1, 2])
    single = torch.cat([run([b]) for b in range(len(prompts))])
    for j in range(steps + 1):
        eb = max(maxerr(batched[b, j], refs[b][j]) for b in range(3))
        e1 = max(maxerr(single[b, j], refs[b][j]) for b in range(3))
        print(f"step {j}: err_batched={eb:.5f} err_b1={e1:.5f}")
        assert eb <= 2 * e1 + 1e-2, (j, eb, e1)


@pytest.mark.parametrize("sampled", [False, True])
def test_generate_batch_graph_equals_eager(bf16_model, sampled):
    from tnn_amd.models.generate import generate_batch
    kw = dict(max_new_tokens=10, seq_len=SEQ, eot_token=None)
    if sampled:
        kw.update(greedy=False, temperature=0.9, top_k=20, top_p=0.9, seed=7)
    prompts = _prompts()
    graph = generate_batch(bf16_model, prompts, use_graph=True, **kw)
    eager = generate_batch(bf16_model, prompts, use_graph=False, **kw)
    assert graph == eager
    for p, o in zip(prompts, graph):
        assert o[:len(p)] == p and len(o) == len(p) + 10


def test_generate_batch_fp32_greedy_matches_recompute():
    from tnn_amd.models.generate import generate, generate_batch
    m = _tiny(torch.float32)
    prompts = _prompts()
    got = generate_batch(m, prompts, max_new_tokens=8, seq_len=SEQ,
                         eot_token=None)
    for p, o in zip(prompts, got):
        assert o == generate(m, p, max_new_tokens=8, seq_len=SEQ,
                             eot_token=None, device=torch.device(DEV))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_generate_batch_capacity_clamp(bf16_model, dtype):
    from tnn_amd.models.generate import generate_batch
    m = bf16_model if dtype == torch.bfloat16 else _tiny(dtype)
    long_p, short_p, other_p = _prompts((SEQ - 2, 3, 9))
    kw = dict(max_new_tokens=8, seq_len=SEQ, eot_token=None)
    both = generate_batch(m, [long_p, short_p], **kw)
    assert len(both[0]) == SEQ and len(both[1]) == 3 + 8
    assert both[0][:SEQ - 2] == long_p
    # the clamped long row did not disturb the short one. fp32: its tokens
    # equal its solo run (exact-token claim, as for generate_graphed). bf16:
    # the solo run takes the M=1 kernels, whose other summation order may
    # flip a near-tie, so the yardstick is the same row slot next to an
    # unclamped neighbour -- the same kernels, bit for bit.
    if dtype == torch.float32:
        assert both[1] == generate_batch(m, [short_p], **kw)[0]
    else:
        assert both[1] == generate_batch(m, [other_p, short_p], **kw)[1]
