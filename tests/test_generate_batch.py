"""Batched ragged decode on CPU (fp32, the eager tensor-driven step):
generate_batch against per-prompt generate, the sampling oracle's rules,
and the per-sequence positional-embedding gather."""

import pytest
import torch

from tnn_amd import ops
from tnn_amd.nn import LayerBuilder
from tnn_amd.models.generate import generate, generate_batch
from tnn_amd.ops.functional import _sample_rules


def _tiny_gpt(vocab=64, dim=32, seq=32):
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
    return _tiny_gpt()


PROMPTS = [[1], [2, 3, 4, 5, 6], [7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18]]
KW = dict(seq_len=32, eot_token=None, use_graph=False)


def test_greedy_rows_match_generate(model):
    got = generate_batch(model, PROMPTS, max_new_tokens=8, **KW)
    for p, g in zip(PROMPTS, got):
        assert g == generate(model, p, max_new_tokens=8, seq_len=32,
                             eot_token=None)
    # state fully restored: a plain forward still works
    assert model(torch.randint(0, 64, (2, 16))).shape == (2, 16, 64)


def test_single_prompt_and_eot(model):
    ref = generate(model, [1, 2, 3], max_new_tokens=10, seq_len=32,
                   eot_token=None)
    assert generate_batch(model, [[1, 2, 3]], max_new_tokens=10, **KW) == [ref]
    eot = ref[5]
    a = generate(model, [1, 2, 3], max_new_tokens=10, seq_len=32,
                 eot_token=eot)
    b = generate_batch(model, [[1, 2, 3], [4]], max_new_tokens=10, seq_len=32,
                       eot_token=eot, use_graph=False)
    assert b[0] == a


def test_top_k_one_is_greedy(model):
    greedy = generate_batch(model, PROMPTS, max_new_tokens=6, **KW)
    k1 = generate_batch(model, PROMPTS, max_new_tokens=6, greedy=False,
                        temperature=0.7, top_k=1, seed=3, **KW)
    assert k1 == greedy


def test_seed_reproduces_and_changes(model):
    kw = dict(max_new_tokens=8, greedy=False, temperature=1.5, top_k=20,
              top_p=0.95, **KW)
    a = generate_batch(model, PROMPTS, seed=11, **kw)
    b = generate_batch(model, PROMPTS, seed=11, **kw)
    c = generate_batch(model, PROMPTS, seed=12, **kw)
    assert a == b
    assert a != c
    for p, g in zip(PROMPTS, a):
        assert g[:len(p)] == p and len(g) == len(p) + 8


def test_chunking_matches_chunks_by_hand(model):
    g = torch.Generator().manual_seed(5)
    prompts = [torch.randint(0, 64, (1 + i % 5,), generator=g).tolist()
               for i in range(18)]
    kw = dict(max_new_tokens=4, greedy=False, temperature=1.2, top_k=10,
              seed=2, **KW)
    whole = generate_batch(model, prompts, **kw)
    by_hand = (generate_batch(model, prompts[:16], **kw)
               + generate_batch(model, prompts[16:], **kw))
    assert whole == by_hand


def test_full_row_returned_unchanged_and_capacity(model):
    full = list(range(32))
    near = list(range(30))
    got = generate_batch(model, [full, [1, 2, 3], near], max_new_tokens=8,
                         **KW)
    assert got[0] == full
    assert len(got[1]) == 3 + 8 and len(got[2]) == 32
    # the clamped row did not disturb its neighbours
    assert got[1] == generate_batch(model, [[1, 2, 3]], max_new_tokens=8,
                                    **KW)[0]
    assert got[2] == generate(model, near, max_new_tokens=2, seq_len=32,
                              eot_token=None)
    assert generate_batch(model, [full], max_new_tokens=8, **KW) == [full]


@pytest.mark.parametrize("kw", [
    dict(prompts=[[1], []]),
    dict(top_p=0.0), dict(top_p=1.5), dict(top_k=-1), dict(temperature=-0.5),
])
def test_invalid_arguments_raise(model, kw):
    args = dict(prompts=[[1, 2]], max_new_tokens=2, greedy=False, **KW)
    args.update(kw)
    with pytest.raises(ValueError):
        generate_batch(model, **args)


def test_sample_oracle_tie_rules():
    # values (= log-weights) with ties at both thresholds
    #   index: 0    1    2    3    4    5    6    7
    z = torch.tensor([[1.0, 3.0, 2.0, 3.0, 2.0, 0.0, 2.0, -1.0]])
    # top_k=3: the third largest value is 2.0 and all three 2.0s stay
    keep, w = _sample_rules(z, 1.0, 3, 1.0)
    assert keep[0].tolist() == [False, True, True, True, True, False, True,
                                False]
    assert torch.all(w[0][~keep[0]] == 0)
    # top_p over everything: p(3.0 pair) = 2e^3 / Z ~ 0.60; adding the 2.0
    # triple reaches ~0.94. top_p = 0.5 keeps the pair, 0.7 the pair + triple.
    Z = torch.exp(z.double()).sum()
    pair = float(2 * torch.exp(torch.tensor(3.0, dtype=torch.float64)) / Z)
    assert 0.5 < pair < 0.7
    keep, _ = _sample_rules(z, 1.0, 0, 0.5)
    assert keep[0].nonzero().flatten().tolist() == [1, 3]
    keep, _ = _sample_rules(z, 1.0, 0, 0.7)
    assert keep[0].nonzero().flatten().tolist() == [1, 2, 3, 4, 6]
    # top-p applies to the renormalised top-k survivors: with top_k=2 the
    # pair alone is the whole mass, so even top_p = 0.99 keeps just the pair
    keep, _ = _sample_rules(z, 1.0, 2, 0.99)
    assert keep[0].nonzero().flatten().tolist() == [1, 3]
    # temperature scales z before the mass is taken
    keep, _ = _sample_rules(z, 0.25, 0, 0.9)
    assert keep[0].nonzero().flatten().tolist() == [1, 3]


def test_sample_oracle_draw_and_greedy():
    z = torch.tensor([[1.0, 3.0, 2.0, 3.0, 2.0, 0.0, 2.0, -1.0]])
    step = torch.zeros(1, dtype=torch.int64)
    # greedy: lowest index among the maxima
    assert ops.sample_logits(z, 0.0, 0, 1.0, 0, step).tolist() == [1]
    assert ops.sample_logits(z, 0.7, 1, 1.0, 0, step).tolist() == [1]
    # explicit u walks the kept CDF in token order: kept = {1, 3}, equal mass
    for u, want in ((1e-6, 1), (0.5, 1), (0.51, 3), (1.0, 3)):
        got = ops.sample_logits(z, 1.0, 0, 0.5, 0, step,
                                u=torch.tensor([u]))
        assert got.tolist() == [want], (u, got)
    # (seed, step) select the draw
    big = torch.randn(64, 200, generator=torch.Generator().manual_seed(1))
    a = ops.sample_logits(big, 1.0, 0, 1.0, 5, step)
    assert torch.equal(a, ops.sample_logits(big, 1.0, 0, 1.0, 5, step))
    assert not torch.equal(a, ops.sample_logits(big, 1.0, 0, 1.0, 6, step))
    assert not torch.equal(a, ops.sample_logits(big, 1.0, 0, 1.0, 5, step + 1))
    with pytest.raises(ValueError):
        ops.sample_logits(z, 1.0, 0, 0.0, 0, step)


def test_positional_embedding_per_sequence_gather():
    from tnn_amd.nn.layers import PositionalEmbedding
    torch.manual_seed(0)
    pe = PositionalEmbedding(16, 8)
    x = torch.randn(3, 1, 8)
    pos = torch.tensor([0, 7, 15])
    pe._pos_tensor = pos
    y = pe(x)
    assert y.shape == (3, 1, 8)
    assert torch.equal(y, x + pe.weight[pos][:, None, :])
    # the shared [1] position keeps its meaning
    pe._pos_tensor = torch.tensor([4])
    assert torch.equal(pe(x[:1]), x[:1] + pe.weight[4])
