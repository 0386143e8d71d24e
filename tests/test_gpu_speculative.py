"""Speculative greedy decode on the GPU: generate_speculative against
generate_batch (fp32, three drafts), graph against eager (bf16), every
emitted bf16 token held to the target's own logit error, BatchedDecoder.verify
against extend, and the caches after a call that raised halfway. The model
is the dim-128 / 2-head / vocab 300 one of test_gpu_decode_session.py with
SEQ 320; prompts of 1, 70, 200 and 310 tokens put the verify steps of the
bf16 runs on the split-KV extend kernel over one to five KV tiles and at the
brim of the cache."""

import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEQ, VOCAB = 320, 300
NEW, K = 12, 4


def _tiny(dtype, seed=3, depth=2):
    from tnn_amd.nn import LayerBuilder
    from tnn_amd.nn.layer import cast_compute_dtype
    torch.manual_seed(seed)
    b = (LayerBuilder((SEQ,)).embedding(VOCAB, 128, "tok")
         .positional_embedding(SEQ, "pos"))
    for i in range(depth):
        b = b.gpt_block(2, 4, flash=(i % 2 == 0), name=f"b{i}")
    m = b.layernorm(name="ln_f").dense(VOCAB, True, "head").build("tiny_gpt")
    if dtype != torch.float32:
        cast_compute_dtype(m, dtype)
    return m.to(DEV).eval()


def _perturbed(model, scale, seed=11):
    """a copy with noise of ``scale`` on the last block's weights"""
    d = copy.deepcopy(model)
    last = max(int(n.split(".")[1]) for n, _ in d.named_parameters()
               if ".attn." in n)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in d.named_parameters():
            if n.startswith(f"layers.{last}."):
                p.add_((torch.randn(p.shape, generator=g) * scale)
                       .to(p.dtype).to(p.device))
    return d


def _drafts(target, dtype):
    return {"copy": copy.deepcopy(target),
            "other": _tiny(dtype, seed=7, depth=1),
            "near": _perturbed(target, 3e-3)}


def _toks(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, VOCAB, (n,), generator=g).tolist()


PROMPTS = [_toks(1, 1), _toks(70, 2), _toks(200, 3), _toks(310, 4)]


@pytest.fixture(scope="module")
def bf16_model():
    return _tiny(torch.bfloat16)


@pytest.fixture(scope="module")
def bf16_drafts(bf16_model):
    return _drafts(bf16_model, torch.bfloat16)


def _spec(target, draft, **kw):
    from tnn_amd.models.generate import generate_speculative
    kw.setdefault("max_new_tokens", NEW)
    return generate_speculative(target, draft, PROMPTS, k=K, seq_len=SEQ,
                                eot_token=None, return_stats=True, **kw)


def _caches_gone(model):
    from tnn_amd.nn.blocks import _MHABase
    return all(m._kv_cache is None for m in model.modules()
               if isinstance(m, _MHABase))


def test_fp32_tokens_equal_generate_batch():
    from tnn_amd.models.generate import generate_batch
    target = _tiny(torch.float32)
    want = generate_batch(copy.deepcopy(target), PROMPTS, max_new_tokens=NEW,
                          seq_len=SEQ, eot_token=None)
    assert [len(w) - len(p) for w, p in zip(want, PROMPTS)] == [
        NEW, NEW, NEW, SEQ - 310]
    for name, draft in _drafts(target, torch.float32).items():
        got, stats = _spec(target, draft)
        print(f"fp32 draft {name}: {stats}")
        assert got == want, name
        if name == "copy":
            assert stats["accepted"] == stats["drafted"]
        assert _caches_gone(target) and _caches_gone(draft)


@pytest.mark.parametrize("name", ["copy", "other", "near"])
def test_bf16_graph_equals_eager(bf16_model, bf16_drafts, name):
    graph = _spec(bf16_model, bf16_drafts[name], use_graph=True)
    eager = _spec(bf16_model, bf16_drafts[name], use_graph=False)
    print(f"bf16 draft {name}: {graph[1]}")
    assert graph == eager
    assert _spec(bf16_model, bf16_drafts[name], use_graph=True) == graph
    assert [len(o) - len(p) for o, p in zip(graph[0], PROMPTS)] == [
        NEW, NEW, NEW, SEQ - 310]


@pytest.mark.parametrize("name", ["copy", "near"])
def test_bf16_tokens_are_near_argmax(bf16_model, bf16_drafts, name):
    """Every emitted token against a CPU fp32 recompute of its context,
    with a bf16 prefill of the same context as yardstick (as
    test_extend_logits_against_recompute): the fp32 logit of the emitted
    token lies within 2 * (2 * err_prefill + 1e-2) of the fp32 maximum."""
    from tnn_amd.models.generate import BatchedDecoder
    from tnn_amd.nn.layer import cast_compute_dtype
    new = 8
    out, _ = _spec(bf16_model, bf16_drafts[name], max_new_tokens=new)
    ref_m = copy.deepcopy(bf16_model).cpu().float()
    cast_compute_dtype(ref_m, torch.float32)
    yard = BatchedDecoder(copy.deepcopy(bf16_model), SEQ)
    try:
        for i in range(new):
            rows = [b for b, p in enumerate(PROMPTS) if len(p) + i < len(out[b])]
            ctx = [out[b][:len(PROMPTS[b]) + i] for b in rows]
            full = yard.prefill(ctx).float().cpu()
            for r, b in enumerate(rows):
                with torch.no_grad():
                    want = ref_m(torch.tensor([ctx[r]]))[0, -1].float()
                ep = (full[r] - want).abs().max().item()
                tok = out[b][len(ctx[r])]
                gap = (want.max() - want[tok]).item()
                print(f"token {i} row {b} len {len(ctx[r])}: gap={gap:.5f} "
                      f"err_prefill={ep:.5f}")
                assert gap <= 2 * (2 * ep + 1e-2), (i, b, gap, ep)
    finally:
        yard.close()


def test_verify_is_the_argmax_of_extend(bf16_model):
    """verify returns, per fed token, the argmax (lowest index among the
    maxima) of what extend returns for the prefix that ends there, and
    advances the positions by the chunk lengths. Row 1 keeps its 16 tokens
    in every extend call and the split count is verify's, so both sides
    run the same kernels on the same shapes and the comparison is exact."""
    from tnn_amd import _C
    from tnn_amd.models.generate import BatchedDecoder
    chunks = [_toks(5, 21), _toks(16, 22), [], _toks(9, 23)]
    ns = _C.ext().attn_extend_splits(4 * 2, SEQ, 16)
    dec = BatchedDecoder(bf16_model, SEQ)
    one = BatchedDecoder(copy.deepcopy(bf16_model), SEQ)

    def pick(lg):
        return int((lg == lg.max()).nonzero()[0])

    try:
        dec.prefill(PROMPTS)
        before = dec.pos.tolist()
        got = dec.verify(chunks)
        assert got.shape == (4, 16) and got.dtype == torch.int64
        assert got.is_cuda
        assert dec.pos.tolist() == [p + len(c) for p, c in zip(before, chunks)]
        got = got.tolist()
        for t in range(9):
            one.prefill(PROMPTS)
            logits = one.extend([chunks[0][:t + 1], chunks[1], [],
                                 chunks[3][:t + 1]], kv_splits=ns).float()
            for b in (0, 3):
                if t < len(chunks[b]):
                    assert got[b][t] == pick(logits[b]), (b, t)
            if t == 8:
                assert got[1][15] == pick(logits[1])
        with pytest.raises(ValueError):          # row 3 has one slot left
            dec.verify([[], [], [], _toks(2, 24)])
    finally:
        dec.close()
        one.close()


def test_caches_are_gone_after_a_failure_halfway(bf16_model, bf16_drafts):
    """the draft takes contexts of up to 256 tokens only: its prefill raises
    after the target's has built caches"""
    draft = copy.deepcopy(bf16_drafts["other"])

    def limit(_, args):
        if args[0].shape[1] > 256:
            raise ValueError("this draft reads at most 256 tokens")

    draft.register_forward_pre_hook(limit)
    with pytest.raises(ValueError, match="256 tokens"):
        _spec(bf16_model, draft)
    assert _caches_gone(bf16_model) and _caches_gone(draft)
    from tnn_amd.nn.layers import PositionalEmbedding
    for m in (bf16_model, draft):
        assert all(p._pos_tensor is None for p in m.modules()
                   if isinstance(p, PositionalEmbedding))
    # and the target decodes as before
    a = _spec(bf16_model, bf16_drafts["other"], max_new_tokens=4)
    b = _spec(bf16_model, bf16_drafts["other"], max_new_tokens=4)
    assert a == b
