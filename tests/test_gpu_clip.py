"""Global-norm gradient clipping on the GPU: the multi-tensor norm kernels
against a float64 oracle, the clipped update kernels against the CPU
optimizer, the skip on a non-finite norm, and hipGraph capture with a
device-resident learning rate."""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from tnn_amd import ops
from tnn_amd.nn import optim

DEV = "cuda"

# Norm tolerance, derived: squares are non-negative (no cancellation). A
# thread chains at most MT_CHUNK/256 = 64 fp32 fmas (one rounding each; the
# bound below also allows a separate multiply rounding) and the block
# reduce is an 8-level tree, so sumsq is off by at most about
# (64 + 9) * 2^-24 = 4.4e-6 relative. The fold of the partials runs in
# double and adds nothing visible; the square root halves the bound to
# 2.2e-6. 1e-5 leaves a 4x margin.
NORM_REL = 1e-5

NUMELS = [1, 3, 7, 64, 1000, 16384, 16385, 40001]
N_TENSORS = 300  # 37.5 cycles x 11 chunks = 413 partials > 256


def relerr(a, b):
    a, b = a.float(), b.float()
    return ((a - b).abs() / (b.abs().clamp_min(1.0))).max().item()


def _oracle(tensors):
    return math.sqrt(sum(t.cpu().double().pow(2).sum().item()
                         for t in tensors))


_CPU_SET = {}


def _cpu_set(kind):
    """~300 CPU gradient tensors, generated once and never modified."""
    if kind not in _CPU_SET:
        g = torch.Generator().manual_seed(7)
        out = []
        for i in range(N_TENSORS):
            t = torch.randn(NUMELS[i % len(NUMELS)], generator=g)
            bf = {"fp32": False, "bf16": True, "mixed": i % 3 == 1}[kind]
            out.append(t.bfloat16() if bf else t)
        _CPU_SET[kind] = out
    return _CPU_SET[kind]


@pytest.mark.parametrize("kind", ["fp32", "bf16", "mixed"])
def test_norm_matches_float64_oracle(kind):
    cpu = _cpu_set(kind)
    gpu = [t.to(DEV) for t in cpu]  # separate allocations: aligned starts
    n1 = ops.grad_global_norm(gpu)
    n2 = ops.grad_global_norm(gpu)
    assert n1.dtype == torch.float32 and n1.dim() == 0 and n1.is_cuda
    ref = _oracle(cpu)
    print(f"{kind}: gpu {n1.item():.9g} oracle {ref:.9g} "
          f"rel {abs(n1.item() - ref) / ref:.3g}")
    assert n1.item() == pytest.approx(ref, rel=NORM_REL)
    assert torch.equal(n1, n2)  # no atomics: bit-identical


@pytest.mark.parametrize("kind", ["fp32", "bf16", "mixed"])
def test_norm_of_views_into_a_slab(kind):
    """Views carved out of one slab per dtype at odd element offsets, as
    GraphedTrainStep hands out grads: span starts that are only 2- or
    4-byte aligned."""
    cpu = _cpu_set(kind)
    slabs, offs = {}, {}
    for dt in {t.dtype for t in cpu}:
        n = sum(t.numel() + 1 for t in cpu if t.dtype == dt) + 1
        slabs[dt] = torch.zeros(n, dtype=dt, device=DEV)
        offs[dt] = 1
    views = []
    for t in cpu:
        o = offs[t.dtype]
        v = slabs[t.dtype][o:o + t.numel()]
        v.copy_(t)
        views.append(v)
        offs[t.dtype] = o + t.numel() + 1  # a gap: starts of either parity
    assert any(v.data_ptr() % 16 for v in views)
    n1 = ops.grad_global_norm(views)
    n2 = ops.grad_global_norm(views)
    ref = _oracle(cpu)
    print(f"{kind} slab: gpu {n1.item():.9g} oracle {ref:.9g} "
          f"rel {abs(n1.item() - ref) / ref:.3g}")
    assert n1.item() == pytest.approx(ref, rel=NORM_REL)
    assert torch.equal(n1, n2)


def test_norm_of_noncontiguous_and_other_dtypes():
    g = torch.Generator().manual_seed(3)
    a = torch.randn(37, 19, generator=g)
    b = torch.randn(501, generator=g).half()
    ref = _oracle([a, b])
    n = ops.grad_global_norm([a.to(DEV).t(), None, b.to(DEV)])
    assert n.item() == pytest.approx(ref, rel=NORM_REL)


# ---------------------------------------------------------------------------
# update kernels against the CPU optimizer with the same max_grad_norm
# ---------------------------------------------------------------------------

# gradients are 2 * N(0,1); the threshold is about half their global norm,
# so every step clips with a coefficient near 0.5 and the clipped values
# stay O(1): an ignored coefficient shows at the 1e-5 level everywhere
G_SCALE = 2.0


def _threshold(shapes):
    return 0.5 * G_SCALE * math.sqrt(sum(math.prod(s) for s in shapes))


def _pair(shapes, dtypes, seed):
    g = torch.Generator().manual_seed(seed)
    cpu, gpu = [], []
    for s, dt in zip(shapes, dtypes):
        init = torch.randn(*s, generator=g).to(dt)
        cpu.append(torch.nn.Parameter(init.clone()))
        gpu.append(torch.nn.Parameter(init.clone().to(DEV)))
    return cpu, gpu


def _run(o_cpu, o_gpu, p_cpu, p_gpu, steps=5, seed=50, grad_dtypes=None):
    g = torch.Generator().manual_seed(seed)
    for i, (a, b) in enumerate(zip(p_cpu, p_gpu)):
        if grad_dtypes and grad_dtypes[i] != a.dtype:
            a.grad_dtype = b.grad_dtype = None  # allow a grad of another dtype
    for _ in range(steps):
        for i, (a, b) in enumerate(zip(p_cpu, p_gpu)):
            dt = grad_dtypes[i] if grad_dtypes else a.dtype
            gr = (torch.randn(a.shape, generator=g) * G_SCALE).to(dt)
            a.grad = gr.clone()
            b.grad = gr.clone().to(DEV)
        norm = _oracle([a.grad for a in p_cpu])
        assert norm > 1.5 * o_cpu.max_grad_norm  # this step clips
        o_cpu.step()
        o_gpu.step()
        assert o_gpu.last_grad_norm.item() == pytest.approx(norm, rel=NORM_REL)
    assert o_gpu.skipped_steps() == 0


def _check_adam_state(o_cpu, o_gpu, n):
    for i in range(n):
        sc, sg = o_cpu.state[i], o_gpu.state[i]
        assert relerr(sg["m"].cpu(), sc["m"]) < 1e-5
        assert relerr(sg["v"].cpu(), sc["v"]) < 1e-5
        # v is a sum of non-negative terms (1-b2) * coef^2 * g^2 (no
        # cancellation), so it also supports an element-wise relative
        # check. Error budget: the kernel forms 1-b2 from the fp32 0.999
        # (off by up to 2^-25, i.e. 3e-5 of 0.001) where the CPU path
        # rounds the double 0.001; the norm is within 2.2e-6 (above), hence
        # coef^2 within 4.6e-6; about ten 2^-24 roundings over 5 steps add
        # 1e-6. Sum 3.6e-5, bound 1e-4. An ignored coefficient is off by a
        # factor 4.
        big = sc["v"] > 1e-6
        rel = ((sg["v"].cpu()[big] - sc["v"][big]).abs() / sc["v"][big]).max()
        print(f"param {i}: max relative error of v {rel.item():.3g}")
        assert rel.item() < 1e-4, rel.item()
        if "master" in sc:
            assert relerr(sg["master"].cpu(), sc["master"]) < 1e-5


MT_SHAPES = [(1000,), (33, 17), (16385,)]  # 3 same-dtype params: one launch


@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_sgd_clipped_matches_cpu(momentum):
    c = _threshold(MT_SHAPES)
    p_cpu, p_gpu = _pair(MT_SHAPES, [torch.float32] * 3, seed=20)
    kw = dict(lr=0.1, momentum=momentum, weight_decay=1e-4,
              nesterov=momentum > 0, max_grad_norm=c)
    o_cpu, o_gpu = optim.SGD(p_cpu, **kw), optim.SGD(p_gpu, **kw)
    _run(o_cpu, o_gpu, p_cpu, p_gpu)
    for a, b in zip(p_cpu, p_gpu):
        assert relerr(b.cpu(), a) < 1e-5


def test_adamw_clipped_multi_tensor_matches_cpu():
    c = _threshold(MT_SHAPES)
    p_cpu, p_gpu = _pair(MT_SHAPES, [torch.float32] * 3, seed=21)
    kw = dict(lr=0.05, weight_decay=0.1, max_grad_norm=c)
    o_cpu, o_gpu = optim.AdamW(p_cpu, **kw), optim.AdamW(p_gpu, **kw)
    _run(o_cpu, o_gpu, p_cpu, p_gpu)
    _check_adam_state(o_cpu, o_gpu, 3)
    for a, b in zip(p_cpu, p_gpu):
        assert relerr(b.cpu(), a) < 1e-5


def test_adamw_clipped_bf16_master_matches_cpu():
    shapes = [(512,), (77,), (33, 5)]
    c = _threshold(shapes)
    p_cpu, p_gpu = _pair(shapes, [torch.bfloat16] * 3, seed=22)
    kw = dict(lr=0.05, max_grad_norm=c)
    o_cpu, o_gpu = optim.AdamW(p_cpu, **kw), optim.AdamW(p_gpu, **kw)
    _run(o_cpu, o_gpu, p_cpu, p_gpu)
    _check_adam_state(o_cpu, o_gpu, 3)
    for a, b in zip(p_cpu, p_gpu):
        assert torch.equal(b.cpu(), a)


def test_adamw_clipped_bf16_multi_chunk_matches_cpu():
    """bf16 params over several chunks, vector and scalar spans."""
    shapes = [(40001,), (16385,), (1000,)]
    c = _threshold(shapes)
    p_cpu, p_gpu = _pair(shapes, [torch.bfloat16] * 3, seed=23)
    kw = dict(lr=0.05, weight_decay=0.01, max_grad_norm=c)
    o_cpu, o_gpu = optim.AdamW(p_cpu, **kw), optim.AdamW(p_gpu, **kw)
    _run(o_cpu, o_gpu, p_cpu, p_gpu)
    _check_adam_state(o_cpu, o_gpu, 3)


def test_adam_clipped_single_tensor_fallback_matches_cpu():
    """One fp32 parameter, one bf16 parameter with a bf16 grad and one fp32
    parameter with a bf16 grad: three groups of one, all single-tensor."""
    shapes = [(777,), (300,), (129,)]
    c = _threshold(shapes)
    p_cpu, p_gpu = _pair(shapes, [torch.float32, torch.bfloat16,
                                  torch.float32], seed=24)
    kw = dict(lr=0.05, weight_decay=0.01, max_grad_norm=c)
    o_cpu, o_gpu = optim.Adam(p_cpu, **kw), optim.Adam(p_gpu, **kw)
    _run(o_cpu, o_gpu, p_cpu, p_gpu,
         grad_dtypes=[torch.float32, torch.bfloat16, torch.bfloat16])
    _check_adam_state(o_cpu, o_gpu, 3)
    assert relerr(p_gpu[0].cpu(), p_cpu[0]) < 1e-5
    assert relerr(p_gpu[2].cpu(), p_cpu[2]) < 1e-5


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_huge_threshold_equals_no_clipping_gpu(kind):
    def mk(ps, c):
        if kind == "sgd":
            return optim.SGD(ps, lr=0.1, momentum=0.9, weight_decay=1e-4,
                             max_grad_norm=c)
        return optim.AdamW(ps, lr=0.05, weight_decay=0.1, max_grad_norm=c)
    shapes = MT_SHAPES + [(129,)]
    dts = [torch.float32] * 3 + [torch.bfloat16]
    _, p1 = _pair(shapes, dts, seed=25)
    _, p2 = _pair(shapes, dts, seed=25)
    a, b = mk(p1, 1e30), mk(p2, 0.0)
    g = torch.Generator().manual_seed(60)
    for _ in range(3):
        for x, y in zip(p1, p2):
            gr = torch.randn(x.shape, generator=g).to(x.dtype).to(DEV)
            x.grad, y.grad = gr.clone(), gr.clone()
        a.step()
        b.step()
    for x, y in zip(p1, p2):
        assert torch.equal(x, y)
    sa, sb = a.state_tensors(), b.state_tensors()
    assert [n for n, _ in sa] == [n for n, _ in sb]
    for (_, x), (_, y) in zip(sa, sb):
        assert torch.equal(x, y)


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_nonfinite_grad_skips_the_step_gpu(kind):
    """An inf in one bf16 grad (data, not a fault): every parameter and all
    state stay bit-identical, the skip is counted, the next step runs."""
    shapes = [(1000,), (33, 17), (16385,), (129,)]
    dts = [torch.bfloat16] * 3 + [torch.float32]  # bf16 group + a single
    _, ps = _pair(shapes, dts, seed=26)
    if kind == "sgd":
        o = optim.SGD(ps, lr=0.1, momentum=0.9, max_grad_norm=1.0)
    else:
        o = optim.AdamW(ps, lr=0.05, weight_decay=0.1, max_grad_norm=1.0)
    g = torch.Generator().manual_seed(61)

    def set_grads(poison):
        for i, p in enumerate(ps):
            gr = torch.randn(p.shape, generator=g).to(p.dtype)
            if poison and i == 1:
                gr[5, 3] = float("inf")
            p.grad = gr.to(DEV)

    set_grads(False)
    o.step()  # creates all state
    before_p = [p.detach().clone() for p in ps]
    before_s = [(n, t.clone()) for n, t in o.state_tensors()]
    set_grads(True)
    o.step()
    assert o.skipped_steps() == 1
    assert not math.isfinite(o.last_grad_norm.item())
    assert o.step_count == 2
    for p, b in zip(ps, before_p):
        assert torch.equal(p, b)
    after_s = o.state_tensors()
    assert [n for n, _ in after_s] == [n for n, _ in before_s]
    for (_, t), (_, b) in zip(after_s, before_s):
        assert torch.equal(t, b)
    set_grads(False)
    o.step()
    assert o.skipped_steps() == 1
    for p, b in zip(ps, before_p):
        assert not torch.equal(p, b)
        assert torch.isfinite(p.float()).all()


# ---------------------------------------------------------------------------
# hipGraph capture
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("max_norm", [0.0, 1.0])
def test_captured_optimizer_step_follows_the_schedule(max_norm):
    """Capture optimizer.step() over static grad buffers with the step
    counter and the learning rate on the device; a twin runs the same
    kernels eagerly. Same kernels, same inputs: exact equality. Without
    lr_dev the graph would replay the learning rate it was captured with."""
    shapes = MT_SHAPES + [(129,)]
    dts = [torch.float32] * 3 + [torch.bfloat16]  # one group + one single
    _, pg = _pair(shapes, dts, seed=27)
    _, pe = _pair(shapes, dts, seed=27)

    def mk(ps):
        o = optim.AdamW(ps, lr=0.02, weight_decay=0.1, max_grad_norm=max_norm)
        o._step_dev = torch.zeros(1, dtype=torch.int64, device=DEV)
        o._lr_dev = torch.full((1,), o.lr, dtype=torch.float32, device=DEV)
        return o

    og, oe = mk(pg), mk(pe)
    static = [torch.zeros_like(p) for p in pg]
    for p, s in zip(pg, static):
        p.grad = s
    gen = torch.Generator().manual_seed(62)

    def schedule(t):  # warm-up then decay: a different value every step
        return 0.02 * min(t / 3.0, 1.0) * 0.9 ** t

    def feed(t):
        for o in (og, oe):
            o.lr = schedule(t)
            o._lr_dev.fill_(o.lr)
            o._step_dev.fill_(t)
        for s, p in zip(static, pe):
            gr = torch.randn(s.shape, generator=gen).to(s.dtype).to(DEV)
            s.copy_(gr)
            p.grad = gr.clone()

    # t = 0 is the warm-up outside the graph (state, descriptors, buffers)
    feed(1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        og.step()
    torch.cuda.current_stream().wait_stream(side)
    oe.step()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        og.step()
    for t in range(2, 7):
        feed(t)
        graph.replay()
        oe.step()
    torch.cuda.synchronize()
    for a, b in zip(pg, pe):
        assert torch.equal(a, b)
    sg, se = og.state_tensors(), oe.state_tensors()
    assert [n for n, _ in sg] == [n for n, _ in se]
    for (_, a), (_, b) in zip(sg, se):
        assert torch.equal(a, b)
    if max_norm:
        assert torch.equal(og.last_grad_norm, oe.last_grad_norm)
        assert og.skipped_steps() == 0


@pytest.mark.parametrize("max_norm", [0.05, 1e3])
def test_graphed_train_step_clips(max_norm):
    """Tiny fp32 dense model, plain SGD with lr = 1: the update IS the
    clipped gradient, so its length is min(norm, max_norm). One threshold
    clips every step, the other never does."""
    from tnn_amd.nn import CrossEntropyLoss, LayerBuilder
    from tnn_amd.utils.graphstep import GraphedTrainStep
    torch.manual_seed(4)
    model = (LayerBuilder(input_shape=(32,), dtype=torch.float32)
             .dense(66, True, "fc1")
             .activation("relu", "r1")
             .dense(10, True, "fc2")
             .build("clip_graph")).to(DEV)
    opt = optim.SGD(model.parameters(), lr=1.0, max_grad_norm=max_norm)
    g = torch.Generator().manual_seed(63)
    x = torch.randn(16, 32, generator=g).to(DEV)
    y = torch.randint(0, 10, (16,), generator=g).to(DEV)
    step = GraphedTrainStep(model, CrossEntropyLoss(), opt, x, y, warmup=2)
    # the second bias/weight views start off a 16-byte boundary
    assert any(p.grad.data_ptr() % 16 for p in opt.params)
    clipped = 0
    for _ in range(3):
        before = [p.detach().clone() for p in opt.params]
        x = torch.randn(16, 32, generator=g).to(DEV)
        y = torch.randint(0, 10, (16,), generator=g).to(DEV)
        step(x, y)
        torch.cuda.synchronize()
        # the grads of this step are still in the slabs
        norm = _oracle(step._grad_slabs)
        assert opt.last_grad_norm.item() == pytest.approx(norm, rel=NORM_REL)
        delta = math.sqrt(sum((p.detach().double() - b.double()).pow(2).sum().item()
                              for p, b in zip(opt.params, before)))
        p_norm = max(_oracle(before), _oracle([p.detach() for p in opt.params]))
        # rounding of p - x in fp32 (half an ulp of every element) plus the
        # norm tolerance on the coefficient
        tol = 2.0 ** -24 * p_norm + 1e-5 * max_norm
        want = min(norm, max_norm)
        print(f"max_norm {max_norm}: norm {norm:.6g} |dp| {delta:.9g} "
              f"want {want:.9g} tol {tol:.3g}")
        assert abs(delta - want) <= tol, (delta, want, tol)
        clipped += norm > max_norm
    assert clipped == (3 if max_norm < 1 else 0)
    assert opt.skipped_steps() == 0
