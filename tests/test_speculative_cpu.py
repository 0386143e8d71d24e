"""generate_speculative on the CPU, fp32: for any draft the result equals
generate_batch on the target, token for token -- ragged prompts, k in
{1, 4, 15}, a row at the brim of seq_len, an EOT in the middle of a round --
and the four argument errors. The model is a dim-64 / 2-head / 2-block GPT
with SEQ 48 and vocabulary 300."""

import copy

import pytest
import torch

from tnn_amd.models.generate import generate_batch, generate_speculative
from tnn_amd.nn import LayerBuilder

SEQ, VOCAB = 48, 300
NEW = 30


def _tiny(seed=3, depth=2, vocab=VOCAB, seq=SEQ):
    torch.manual_seed(seed)
    b = (LayerBuilder((seq,)).embedding(vocab, 64, "tok")
         .positional_embedding(seq, "pos"))
    for i in range(depth):
        b = b.gpt_block(2, 4, flash=(i % 2 == 0), name=f"b{i}")
    return (b.layernorm(name="ln_f").dense(vocab, True, "head")
            .build("tiny_gpt").eval())


def _perturbed(model, scale, seed=11):
    """A copy with noise of ``scale`` on the last block's weights."""
    d = copy.deepcopy(model)
    last = max(int(n.split(".")[1]) for n, _ in d.named_parameters()
               if ".attn." in n)
    torch.manual_seed(seed)
    with torch.no_grad():
        for n, p in d.named_parameters():
            if n.startswith(f"layers.{last}."):
                p.add_(torch.randn_like(p) * scale)
    return d


def _toks(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, VOCAB, (n,), generator=g).tolist()


PROMPTS = [_toks(1, 1), _toks(5, 2), _toks(12, 3)]


@pytest.fixture(scope="module")
def target():
    return _tiny()


@pytest.fixture(scope="module")
def drafts(target):
    return {"copy": copy.deepcopy(target),
            "other": _tiny(seed=7, depth=1),
            "near": _perturbed(target, 3e-3)}


@pytest.fixture(scope="module")
def reference(target):
    return generate_batch(target, PROMPTS, max_new_tokens=NEW, seq_len=SEQ,
                          eot_token=None, use_graph=False)


def _spec(target, draft, prompts=PROMPTS, new=NEW, k=4, eot=None):
    return generate_speculative(target, draft, prompts, max_new_tokens=new,
                                k=k, seq_len=SEQ, eot_token=eot,
                                use_graph=False, return_stats=True)


@pytest.mark.parametrize("k", [1, 4, 15])
@pytest.mark.parametrize("name", ["copy", "other", "near"])
def test_equals_generate_batch(target, drafts, reference, name, k):
    out, stats = _spec(target, drafts[name], k=k)
    assert out == reference
    assert stats["rounds"] >= 1
    for d, a in zip(stats["drafted"], stats["accepted"]):
        assert 0 <= a <= d
    if name == "copy":
        assert stats["accepted"] == stats["drafted"]
        # every round but the last yields k + 1 tokens for every row
        assert stats["rounds"] == -(-(NEW - 1) // (k + 1))


def test_partial_acceptance(target, drafts, reference):
    """The perturbed draft is right often, not always: the acceptance rate
    (accepted / drafted, over all rows) lies strictly inside (0.2, 0.8)."""
    out, stats = _spec(target, drafts["near"], k=4)
    rate = sum(stats["accepted"]) / sum(stats["drafted"])
    print(f"acceptance with the perturbed draft: {rate:.3f} {stats}")
    assert out == reference
    assert 0.2 < rate < 0.8


def test_plain_return_without_stats(target, drafts, reference):
    out = generate_speculative(target, drafts["copy"], PROMPTS,
                               max_new_tokens=NEW, k=4, seq_len=SEQ,
                               eot_token=None, use_graph=False)
    assert out == reference


@pytest.mark.parametrize("name", ["copy", "other", "near"])
def test_row_at_the_brim(target, drafts, name):
    """A prompt 3 tokens short of seq_len with k = 4 (its verify chunk is
    cut), one that fills seq_len (returned unchanged), and a short one
    that goes on alone."""
    prompts = [_toks(SEQ - 3, 4), _toks(SEQ, 5), _toks(2, 6)]
    ref = generate_batch(target, prompts, max_new_tokens=NEW, seq_len=SEQ,
                         eot_token=None, use_graph=False)
    out, stats = _spec(target, drafts[name], prompts=prompts, k=4)
    assert out == ref
    assert len(out[0]) == SEQ and out[1] == prompts[1]
    assert stats["drafted"][1] == 0


@pytest.mark.parametrize("name", ["copy", "other", "near"])
def test_eot_mid_round(target, drafts, reference, name):
    """An EOT that the target emits inside a round (with the copy draft
    and k = 4 a round covers new tokens 1..5, 6..10, ...): that row stops
    there, its neighbours go on."""
    row, idx = next((r, i) for r in range(len(PROMPTS))
                    for i in range(2, NEW)
                    if (i - 1) % 5 in (1, 2, 3)
                    and reference[r][len(PROMPTS[r]) + i]
                    not in reference[r][len(PROMPTS[r]):len(PROMPTS[r]) + i])
    eot = reference[row][len(PROMPTS[row]) + idx]
    ref = generate_batch(target, PROMPTS, max_new_tokens=NEW, seq_len=SEQ,
                         eot_token=eot, use_graph=False)
    assert len(ref[row]) == len(PROMPTS[row]) + idx + 1
    assert any(len(r) == len(p) + NEW for r, p in zip(ref, PROMPTS))
    out, _ = _spec(target, drafts[name], k=4, eot=eot)
    assert out == ref


def test_max_new_tokens_of_one(target, drafts):
    ref = generate_batch(target, PROMPTS, max_new_tokens=1, seq_len=SEQ,
                         eot_token=None, use_graph=False)
    out, stats = _spec(target, drafts["copy"], new=1)
    assert out == ref and stats["rounds"] == 0


def test_more_prompts_than_one_batch(target, drafts):
    prompts = [_toks(1 + i % 5, 20 + i) for i in range(18)]
    ref = generate_batch(target, prompts, max_new_tokens=6, seq_len=SEQ,
                         eot_token=None, use_graph=False)
    out, stats = _spec(target, drafts["near"], prompts=prompts, new=6)
    assert out == ref and len(stats["drafted"]) == 18


def _caches_gone(model):
    from tnn_amd.nn.blocks import _MHABase
    return all(m._kv_cache is None for m in model.modules()
               if isinstance(m, _MHABase))


@pytest.mark.parametrize("what", ["vocab", "positions", "k0", "k16", "empty"])
def test_value_errors(target, drafts, what):
    draft, prompts, k = drafts["copy"], PROMPTS, 4
    if what == "vocab":
        draft = _tiny(vocab=VOCAB + 1)
    elif what == "positions":
        draft = _tiny(seq=SEQ - 1)
    elif what == "k0":
        k = 0
    elif what == "k16":
        k = 16
    else:
        prompts = [PROMPTS[0], []]
    with pytest.raises(ValueError):
        generate_speculative(target, draft, prompts, max_new_tokens=4, k=k,
                             seq_len=SEQ, eot_token=None, use_graph=False)
    assert _caches_gone(target) and _caches_gone(draft)


def test_caches_closed_after_a_run(target, drafts):
    _spec(target, drafts["other"], new=4)
    assert _caches_gone(target) and _caches_gone(drafts["other"])
