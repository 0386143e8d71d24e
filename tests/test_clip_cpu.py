"""Global-norm gradient clipping, CPU path: parity with
torch.nn.utils.clip_grad_norm_ + torch.optim, the skip on a non-finite
norm, and the config surface."""

import pytest
import torch

from tnn_amd import ops
from tnn_amd.nn import optim
from tnn_amd.nn.train import TrainingConfig

SHAPES = [(7,), (5, 3), (2, 3, 4)]


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(*s, generator=g)) for s in SHAPES]


def _grads(step):
    g = torch.Generator().manual_seed(100 + step)
    return [torch.randn(*s, generator=g) for s in SHAPES]


def _global_norm(grads):
    return torch.sqrt(sum(g.double().pow(2).sum() for g in grads))


CASES = {
    "sgd": (lambda ps, c: optim.SGD(ps, lr=0.1, max_grad_norm=c),
            lambda ps: torch.optim.SGD(ps, lr=0.1)),
    "sgd_momentum": (
        lambda ps, c: optim.SGD(ps, lr=0.1, momentum=0.9, weight_decay=1e-2,
                                max_grad_norm=c),
        lambda ps: torch.optim.SGD(ps, lr=0.1, momentum=0.9,
                                   weight_decay=1e-2)),
    "adamw": (
        lambda ps, c: optim.AdamW(ps, lr=0.01, weight_decay=0.1,
                                  max_grad_norm=c),
        lambda ps: torch.optim.AdamW(ps, lr=0.01, weight_decay=0.1,
                                     betas=(0.9, 0.999), eps=1e-8)),
}


# the gradients have 46 N(0,1) elements: norm about 6.8. 0.5 always clips,
# 100 never does (asserted below, not assumed)
@pytest.mark.parametrize("c,clips", [(0.5, True), (100.0, False)])
@pytest.mark.parametrize("kind", list(CASES))
def test_clip_matches_torch(kind, c, clips):
    mk_ours, mk_ref = CASES[kind]
    p1, p2 = _params(), _params()
    ours, ref = mk_ours(p1, c), mk_ref(p2)
    for t in range(5):
        gs = _grads(t)
        norm = _global_norm(gs)
        assert (norm > c) == clips
        for a, b, g in zip(p1, p2, gs):
            a.grad, b.grad = g.clone(), g.clone()
        ours.step()
        torch.nn.utils.clip_grad_norm_(p2, c)
        ref.step()
        assert ours.last_grad_norm.item() == pytest.approx(norm.item(), rel=1e-6)
        # the gradients themselves are not modified
        for a, g in zip(p1, gs):
            assert torch.equal(a.grad, g)
    for a, b in zip(p1, p2):
        # tolerance of test_adam_matches_torch / test_adamw_matches_torch
        assert torch.allclose(a, b, atol=1e-6)
    assert ours.skipped_steps() == 0


def test_adam_moments_see_the_coefficient():
    """Adam's parameters barely depend on the gradient scale, its moments
    do: m = (1-b1) * coef * g after one step."""
    ps = _params()
    o = optim.Adam(ps, lr=1e-3, max_grad_norm=0.5)
    gs = _grads(0)
    for p, g in zip(ps, gs):
        p.grad = g.clone()
    o.step()
    coef = 0.5 / (_global_norm(gs).item() + 1e-6)
    for i, g in enumerate(gs):
        assert torch.allclose(o.state[i]["m"], 0.1 * coef * g, atol=1e-7)
        assert torch.allclose(o.state[i]["v"], 0.001 * (coef * g) ** 2,
                              atol=1e-9)


@pytest.mark.parametrize("kind", list(CASES))
def test_huge_threshold_equals_no_clipping(kind):
    mk_ours, _ = CASES[kind]
    p1, p2 = _params(), _params()
    a, b = mk_ours(p1, 1e30), mk_ours(p2, 0.0)
    for t in range(3):
        for x, y, g in zip(p1, p2, _grads(t)):
            x.grad, y.grad = g.clone(), g.clone()
        a.step()
        b.step()
    for x, y in zip(p1, p2):
        assert torch.equal(x, y)
    for (na, ta), (nb, tb) in zip(a.state_tensors(), b.state_tensors()):
        assert na == nb and torch.equal(ta, tb)
    assert b.last_grad_norm is None


@pytest.mark.parametrize("kind", list(CASES))
def test_nonfinite_grad_skips_the_step(kind):
    mk_ours, _ = CASES[kind]
    ps = _params()
    o = mk_ours(ps, 1.0)
    for p, g in zip(ps, _grads(0)):
        p.grad = g.clone()
    o.step()  # creates all state
    before_p = [p.detach().clone() for p in ps]
    before_s = [(n, t.clone()) for n, t in o.state_tensors()]
    gs = _grads(1)
    gs[1][2, 1] = float("inf")
    for p, g in zip(ps, gs):
        p.grad = g.clone()
    o.step()
    assert o.skipped_steps() == 1
    assert not torch.isfinite(o.last_grad_norm)
    # step_count advances on a skipped step (documented)
    assert o.step_count == 2
    for p, b in zip(ps, before_p):
        assert torch.equal(p, b)
    after_s = o.state_tensors()
    assert [n for n, _ in after_s] == [n for n, _ in before_s]
    for (_, t), (_, b) in zip(after_s, before_s):
        assert torch.equal(t, b)
    # the next finite step updates normally
    for p, g in zip(ps, _grads(2)):
        p.grad = g.clone()
    o.step()
    assert o.skipped_steps() == 1
    for p, b in zip(ps, before_p):
        assert not torch.equal(p, b)
        assert torch.isfinite(p).all()


def test_noncontiguous_grad_and_missing_grad():
    c = 0.5
    p1, p2 = _params(), _params()
    ours = optim.SGD(p1, lr=0.1, max_grad_norm=c)
    ref = torch.optim.SGD(p2, lr=0.1)
    gs = _grads(0)
    nc = torch.randn(3, 5, generator=torch.Generator().manual_seed(5)).t()
    assert not nc.is_contiguous() and nc.shape == SHAPES[1]
    p1[0].grad, p2[0].grad = gs[0].clone(), gs[0].clone()
    p1[1].grad, p2[1].grad = nc, nc.clone()
    p1[2].grad = p2[2].grad = None
    untouched = p1[2].detach().clone()
    ours.step()
    torch.nn.utils.clip_grad_norm_(p2, c)
    ref.step()
    assert ours.last_grad_norm.item() == pytest.approx(
        _global_norm([gs[0], nc]).item(), rel=1e-6)
    for a, b in zip(p1, p2):
        assert torch.allclose(a, b, atol=1e-6)
    assert torch.equal(p1[2], untouched)


def test_config_round_trip():
    ps = _params()
    for mk in (lambda **k: optim.SGD(ps, lr=0.1, momentum=0.9, **k),
               lambda **k: optim.Adam(ps, **k),
               lambda **k: optim.AdamW(ps, weight_decay=0.1, **k)):
        plain = mk()
        assert "max_grad_norm" not in plain.get_config()
        assert optimizer_round_trip(plain, ps).max_grad_norm == 0.0
        clipped = mk(max_grad_norm=0.25)
        cfg = clipped.get_config()
        assert cfg["max_grad_norm"] == 0.25
        again = optimizer_round_trip(clipped, ps)
        assert type(again) is type(clipped)
        assert again.get_config() == cfg
    # honoured, not only stored
    o = optim.optimizer_from_config(
        {"type": "sgd", "lr": 1.0, "max_grad_norm": 0.25}, ps)
    before = [p.detach().clone() for p in ps]
    for p, g in zip(ps, _grads(0)):
        p.grad = g.clone()
    o.step()
    delta = torch.sqrt(sum((p.detach() - b).double().pow(2).sum()
                           for p, b in zip(ps, before)))
    assert delta.item() == pytest.approx(0.25, rel=1e-4)
    with pytest.raises(ValueError):
        optim.SGD(ps, lr=0.1, max_grad_norm=-1.0)


def optimizer_round_trip(o, ps):
    return optim.optimizer_from_config(o.get_config(), ps)


def test_training_config_reads_env(monkeypatch):
    monkeypatch.delenv("MAX_GRAD_NORM", raising=False)
    assert TrainingConfig.from_env().max_grad_norm == 0.0
    monkeypatch.setenv("MAX_GRAD_NORM", "1.5")
    assert TrainingConfig.from_env().max_grad_norm == 1.5


def test_grad_global_norm_cpu():
    gs = _grads(3) + [None]
    n = ops.grad_global_norm(gs)
    assert n.dtype == torch.float32 and n.dim() == 0
    assert n.item() == pytest.approx(_global_norm(gs[:3]).item(), rel=1e-6)
