"""Multi-turn batched decode on the CPU (fp32, the torch form of extend
attention and the eager step): BatchedDecoder.open / extend / rewind against
prefill and full recomputes, and DecodeSession's greedy contract."""

import copy

import pytest
import torch

from tnn_amd.nn import LayerBuilder
from tnn_amd.models.generate import (BatchedDecoder, DecodeSession,
                                     generate_batch)

VOCAB, SEQ = 64, 32


def _tiny_gpt(vocab=VOCAB, dim=32, seq=SEQ):
    return (LayerBuilder((seq,))
            .embedding(vocab, dim, "tok")
            .positional_embedding(seq, "pos")
            .gpt_block(4, 2, flash=True, name="b0")
            .gpt_block(4, 2, flash=False, name="b1")
            .layernorm(name="ln_f")
            .dense(vocab, True, "head")
            .build("tiny_gpt"))


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    return _tiny_gpt().eval()


@pytest.fixture(scope="module")
def ref(model):
    """the same weights in a model of its own: a live decoder keeps its
    model in cache mode, so recomputes and generate_batch run on this one"""
    return copy.deepcopy(model)


def _toks(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, VOCAB, (n,), generator=g).tolist()


PROMPTS = [_toks(1, 1), _toks(5, 2), _toks(12, 3)]


def _recompute(ref, ids):
    """logits after the last token of ids, by a plain full forward"""
    with torch.no_grad():
        return ref(torch.tensor([ids]))[0, -1]


def maxerr(a, b):
    return (a - b).abs().max().item()


def test_open_extend_matches_prefill(model):
    dec = BatchedDecoder(model, SEQ)
    try:
        want = dec.prefill(PROMPTS).clone()
        pos = dec.pos.tolist()
        dec.open(3)
        assert dec.pos.tolist() == [0, 0, 0]
        got = dec.extend(PROMPTS)
        assert got.shape == want.shape
        assert maxerr(got, want) < 1e-4
        assert dec.pos.tolist() == pos == [1, 5, 12]
    finally:
        dec.close()
    # state fully restored: a plain forward still works
    assert model(torch.randint(0, VOCAB, (2, 16))).shape == (2, 16, VOCAB)


def test_extend_with_an_idle_row(model, ref):
    chunks = [_toks(3, 4), [], _toks(7, 5)]
    dec = BatchedDecoder(model, SEQ)
    try:
        dec.prefill(PROMPTS)
        a1 = dec._attns[0]._kv_cache
        k_before = [a._kv_cache["k"][1, :, :5].clone() for a in dec._attns]
        v_before = [a._kv_cache["v"][1, :, :5].clone() for a in dec._attns]
        got = dec.extend(chunks)
        assert torch.isfinite(got).all()
        for b in (0, 2):
            assert maxerr(got[b], _recompute(ref, PROMPTS[b] + chunks[b])) \
                < 1e-4
        assert dec.pos.tolist() == [4, 5, 19]
        for a, k0, v0 in zip(dec._attns, k_before, v_before):
            assert torch.equal(a._kv_cache["k"][1, :, :5], k0)
            assert torch.equal(a._kv_cache["v"][1, :, :5], v0)
        assert a1 is dec._attns[0]._kv_cache       # same live caches
        nxt = [9, 8, 7]
        step = dec.step(nxt)
        for b in range(3):
            ids = PROMPTS[b] + chunks[b] + [nxt[b]]
            assert maxerr(step[b], _recompute(ref, ids)) < 1e-4
        assert dec.pos.tolist() == [5, 6, 20]
    finally:
        dec.close()


def test_rewind_then_another_chunk_equals_a_fresh_decoder(model):
    first = [_toks(4, 6), _toks(2, 7), _toks(6, 8)]
    second = [_toks(5, 9), _toks(3, 10), _toks(1, 11)]
    dec = BatchedDecoder(model, SEQ)
    try:
        dec.prefill(PROMPTS)
        dec.extend(first)
        dec.rewind([len(p) for p in PROMPTS])      # drop the turn
        assert dec.pos.tolist() == [1, 5, 12]
        got = dec.extend(second)
        dec.open(3)
        want = dec.extend([p + c for p, c in zip(PROMPTS, second)])
        assert maxerr(got, want) < 1e-4
        with pytest.raises(ValueError):
            dec.rewind([0, 0, SEQ + 1])
    finally:
        dec.close()


def test_extend_capacity_raises_and_changes_nothing(model, ref):
    dec = BatchedDecoder(model, SEQ)
    try:
        dec.prefill(PROMPTS)
        k0 = dec._attns[0]._kv_cache["k"].clone()
        with pytest.raises(ValueError):
            dec.extend([[1], [2] * (SEQ - 4), [3]])      # 5 + 28 > 32
        assert dec.pos.tolist() == [1, 5, 12]
        assert torch.equal(dec._attns[0]._kv_cache["k"], k0)
        with pytest.raises(ValueError):
            dec.extend([[1], [2]])                       # wrong row count
        got = dec.extend([[1], [2] * (SEQ - 5), [3]])    # exactly full
        assert maxerr(got[1], _recompute(ref, PROMPTS[1] + [2] * (SEQ - 5))) \
            < 1e-4
    finally:
        dec.close()
    with pytest.raises(RuntimeError):
        dec.extend([[1]])


def _contract(ref, before, chunks, got, **kw):
    for b, chunk in enumerate(chunks):
        if not chunk:
            assert got[b] == []
            continue
        full = before[b] + chunk
        want = generate_batch(ref, [full], use_graph=False, **kw)[0]
        assert got[b] == want[len(full):], (b, got[b], want[len(full):])


def test_session_greedy_contract_over_three_calls(model, ref):
    kw = dict(max_new_tokens=6, seq_len=SEQ, eot_token=None)
    sess = DecodeSession(model, 3, seq_len=SEQ)
    try:
        # 1: all rows active
        before = [list(c) for c in sess.context]
        got = sess.generate(PROMPTS, max_new_tokens=6, eot_token=None,
                            use_graph=False)
        _contract(ref, before, PROMPTS, got, **kw)
        assert all(len(g) == 6 for g in got)
        assert sess.context == [p + g for p, g in zip(PROMPTS, got)]
        # 2: row 1 idle
        chunks = [_toks(3, 12), [], _toks(2, 13)]
        before = [list(c) for c in sess.context]
        got = sess.generate(chunks, max_new_tokens=6, eot_token=None,
                            use_graph=False)
        _contract(ref, before, chunks, got, **kw)
        assert sess.context[1] == before[1]
        # 3: row 0 reset and refilled, row 1 woken up, row 2 runs into the
        # end of the cache (12 + 6 + 2 + 6 + 3 = 29 of 32: 3 tokens left)
        sess.reset([0])
        assert sess.context[0] == []
        chunks = [_toks(4, 14), _toks(2, 15), _toks(3, 16)]
        before = [list(c) for c in sess.context]
        got = sess.generate(chunks, max_new_tokens=6, eot_token=None,
                            use_graph=False)
        _contract(ref, before, chunks, got, **kw)
        assert len(got[2]) == 3 and len(sess.context[2]) == SEQ
        with pytest.raises(ValueError):
            sess.generate([[], [], [1]])
    finally:
        sess.close()


def test_session_eot_truncation_and_rewind(model, ref):
    """the tokens the shared steps produce past a row's EOT are dropped
    from the context and dead in the cache: the next turn matches a
    generate_batch on the truncated context"""
    probe = generate_batch(ref, [PROMPTS[1]], max_new_tokens=8, seq_len=SEQ,
                           eot_token=None, use_graph=False)[0][5:]
    eot = probe[2]
    kw = dict(max_new_tokens=8, seq_len=SEQ, eot_token=eot)
    sess = DecodeSession(model, 2, seq_len=SEQ)
    try:
        first = [PROMPTS[1], PROMPTS[2]]
        got = sess.generate(first, max_new_tokens=8, eot_token=eot,
                            use_graph=False)
        _contract(ref, [[], []], first, got, **kw)
        assert got[0][-1] == eot and len(got[0]) <= 3
        chunks = [_toks(3, 17), _toks(1, 18)]
        before = [list(c) for c in sess.context]
        got = sess.generate(chunks, max_new_tokens=8, eot_token=eot,
                            use_graph=False)
        _contract(ref, before, chunks, got, **kw)
    finally:
        sess.close()


def test_session_rewind_drops_a_turn(model, ref):
    kw = dict(max_new_tokens=4, seq_len=SEQ, eot_token=None)
    sess = DecodeSession(model, 2, seq_len=SEQ)
    try:
        first = [PROMPTS[1], PROMPTS[2]]
        sess.generate(first, use_graph=False, **{k: v for k, v in kw.items()
                                                 if k != "seq_len"})
        kept = [len(c) for c in sess.context]
        sess.generate([_toks(3, 19), _toks(2, 20)], max_new_tokens=4,
                      eot_token=None, use_graph=False)
        sess.rewind(kept)
        assert [len(c) for c in sess.context] == kept
        chunks = [_toks(2, 21), _toks(5, 22)]
        before = [list(c) for c in sess.context]
        got = sess.generate(chunks, max_new_tokens=4, eot_token=None,
                            use_graph=False)
        _contract(ref, before, chunks, got, **kw)
        with pytest.raises(ValueError):
            sess.rewind([99, 0])
    finally:
        sess.close()
