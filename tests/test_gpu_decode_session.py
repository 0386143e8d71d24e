"""Multi-turn batched decode on the GPU: BatchedDecoder.extend (flash extend
attention over the live caches) against a CPU fp32 recompute with the
prefill route as yardstick, and DecodeSession against generate_batch, graph
against eager. The model is the dim-128 / 2-head / SEQ 64 / vocab 300 one of
test_gpu_decode_batch.py."""

import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEQ, VOCAB = 64, 300


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


def _toks(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, VOCAB, (n,), generator=g).tolist()


def maxerr(a, b):
    return (a.float() - b.float()).abs().max().item()


def test_extend_logits_against_recompute(bf16_model):
    """Contexts grow by prefill, then extend, then extend, per row 1+17+3,
    5+0+20 and 12+16+0 tokens. Every stage against a CPU fp32 recompute;
    the yardstick is the parent's route, a prefill of the full context:
    err_extend <= 2 * err_prefill_of_full_context + 1e-2."""
    from tnn_amd.models.generate import BatchedDecoder
    from tnn_amd.nn.layer import cast_compute_dtype
    stages = [[_toks(1, 1), _toks(5, 2), _toks(12, 3)],
              [_toks(17, 4), [], _toks(16, 5)],
              [_toks(3, 6), _toks(20, 7), []]]
    ref_m = copy.deepcopy(bf16_model).cpu().float()
    cast_compute_dtype(ref_m, torch.float32)

    def ref(ids):
        with torch.no_grad():
            return ref_m(torch.tensor([ids]))[0, -1].float()

    dec = BatchedDecoder(bf16_model, SEQ)
    yard = BatchedDecoder(copy.deepcopy(bf16_model), SEQ)
    try:
        ctx = [list(p) for p in stages[0]]
        got = dec.prefill(ctx).float().cpu()
        for s, chunks in enumerate(stages):
            if s > 0:
                got = dec.extend(chunks).float().cpu()
                ctx = [c + ch for c, ch in zip(ctx, chunks)]
            assert dec.pos.tolist() == [len(c) for c in ctx]
            full = yard.prefill(ctx).float().cpu()
            for b in range(3):
                if not chunks[b]:
                    assert torch.isfinite(got[b]).all()
                    continue
                want = ref(ctx[b])
                ee, ep = maxerr(got[b], want), maxerr(full[b], want)
                print(f"stage {s} row {b} len {len(ctx[b])}: "
                      f"err_extend={ee:.5f} err_prefill={ep:.5f}")
                assert ee <= 2 * ep + 1e-2, (s, b, ee, ep)
        # the caches stay good for single-token steps
        nxt = [4, 5, 6]
        step = dec.step(nxt).float().cpu()
        stepy = yard.step(nxt).float().cpu()
        for b in range(3):
            want = ref(ctx[b] + [nxt[b]])
            ee, ep = maxerr(step[b], want), maxerr(stepy[b], want)
            print(f"step row {b}: err_extend={ee:.5f} err_prefill={ep:.5f}")
            assert ee <= 2 * ep + 1e-2, (b, ee, ep)
    finally:
        dec.close()
        yard.close()


TURNS = [[_toks(1, 11), _toks(5, 12), _toks(12, 13)],
         [_toks(4, 14), [], _toks(9, 15)],
         [_toks(2, 16), _toks(6, 17), _toks(1, 18)]]


def _session_run(model, **kw):
    from tnn_amd.models.generate import DecodeSession
    sess = DecodeSession(model, 3, seq_len=SEQ)
    try:
        out = []
        for t, chunks in enumerate(TURNS):
            if t == 2:
                sess.reset([0])
            out.append(sess.generate(chunks, max_new_tokens=6, eot_token=None,
                                     **kw))
        return out, [list(c) for c in sess.context]
    finally:
        sess.close()


def test_session_fp32_tokens_equal_generate_batch():
    from tnn_amd.models.generate import DecodeSession, generate_batch
    m = _tiny(torch.float32)
    ref_m = copy.deepcopy(m)
    sess = DecodeSession(m, 3, seq_len=SEQ)
    try:
        for t, chunks in enumerate(TURNS):
            if t == 2:
                sess.reset([0])
            before = [list(c) for c in sess.context]
            got = sess.generate(chunks, max_new_tokens=6, eot_token=None)
            for b, chunk in enumerate(chunks):
                if not chunk:
                    assert got[b] == [] and sess.context[b] == before[b]
                    continue
                full = before[b] + chunk
                want = generate_batch(ref_m, [full], max_new_tokens=6,
                                      seq_len=SEQ, eot_token=None)[0]
                assert got[b] == want[len(full):], (t, b)
                assert len(got[b]) == 6
    finally:
        sess.close()


@pytest.mark.parametrize("sampled", [False, True])
def test_session_graph_equals_eager(bf16_model, sampled):
    kw = {}
    if sampled:
        kw.update(greedy=False, temperature=0.9, top_k=20, top_p=0.9, seed=7)
    graph, ctx_g = _session_run(bf16_model, use_graph=True, **kw)
    eager, ctx_e = _session_run(bf16_model, use_graph=False, **kw)
    assert graph == eager and ctx_g == ctx_e
    again, _ = _session_run(bf16_model, use_graph=True, **kw)   # one seed
    assert again == graph
    for turn, chunks in zip(graph, TURNS):
        assert [len(o) for o in turn] == [6 if c else 0 for c in chunks]
