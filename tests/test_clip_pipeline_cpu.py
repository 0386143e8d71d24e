"""Gradient clipping over a 2-rank gloo pipeline: stages own disjoint
parameters, so the clipping norm has to be the global one (local sum of
squares all-reduced before the coefficient is derived). The pipeline must
match single-process micro-batched training with the same max_grad_norm,
and every rank must report the global norm, not its own stage's."""

import math
import os

import pytest
import torch
import torch.multiprocessing as mp

from tnn_amd.nn import LayerBuilder, CrossEntropyLoss, SGD

# far below the gradient norms of this model (about 1): clips every step,
# asserted on the reference norms below
MAX_NORM = 0.05
OPT_CFG = {"type": "sgd", "lr": 0.1, "max_grad_norm": MAX_NORM}


def _build_model(seed=0):
    torch.manual_seed(seed)
    return (LayerBuilder((8, 8, 3))
            .conv2d(8, 3, 3, 1, 1, 1, 1, True, "c1")
            .batchnorm(relu=True, name="b1")
            .conv2d(8, 3, 3, 1, 1, 1, 1, True, "c2")
            .batchnorm(relu=True, name="b2")
            .maxpool2d(2, 2)
            .flatten()
            .dense(16, True, "fc1")
            .activation("relu", "r1")
            .dense(4, True, "fc2")
            .build("pipe_test"))


def _data(num_batches=3, batch=16, seed=42):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(batch, 8, 8, 3, generator=g),
             torch.randint(0, 4, (batch,), generator=g))
            for _ in range(num_batches)]


def _reference(M=4):
    """Single-process with the same micro-batch split + grad accumulation."""
    model = _build_model()
    crit = CrossEntropyLoss()
    opt = SGD(model.parameters(), lr=OPT_CFG["lr"], max_grad_norm=MAX_NORM)
    losses, norms = [], []
    for x, y in _data():
        total = 0.0
        opt.zero_grad()
        for mx, my in zip(x.chunk(M), y.chunk(M)):
            loss = crit(model(mx), my) / M
            loss.backward()
            total += loss.item()
        opt.step()
        losses.append(total)
        norms.append(opt.last_grad_norm.item())
    return losses, norms


def _worker(rank, world, tmpdir):
    os.environ.update({
        "RANK": str(rank), "WORLD_SIZE": str(world), "LOCAL_RANK": str(rank),
    })
    import torch.distributed as dist
    dist.init_process_group(
        "gloo", init_method=f"file://{tmpdir}/pg_init", rank=rank,
        world_size=world)
    from tnn_amd.parallel import Communicator, PipelineEngine
    comm = Communicator()
    model = _build_model() if rank == 0 else None
    engine = PipelineEngine(model, comm, input_shape=(8, 8, 3),
                            num_microbatches=4, optimizer_config=OPT_CFG,
                            device=torch.device("cpu"), sync_weights=True)
    assert engine.optimizer.max_grad_norm == MAX_NORM
    # record this rank's own sum of squares as it enters the reduction
    local_sumsq = []
    reduce_ = engine.optimizer.norm_reduce
    assert reduce_ is not None

    def recording_reduce(t):
        local_sumsq.append(float(t[0]))
        return reduce_(t)

    engine.optimizer.norm_reduce = recording_reduce
    losses, norms = [], []
    for x, y in _data():
        stats = engine.broadcast_stats(engine.train_batch(x, y))
        losses.append(stats["loss"])
        norms.append(engine.optimizer.last_grad_norm.item())
    torch.save((losses, norms, [math.sqrt(s) for s in local_sumsq]),
               os.path.join(tmpdir, f"result_{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_pipeline_clips_by_the_global_norm(tmp_path):
    ref_losses, ref_norms = _reference()
    assert all(n > MAX_NORM for n in ref_norms), ref_norms
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_worker, args=(r, 2, str(tmp_path)))
             for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=180)
        assert p.exitcode == 0
    results = [torch.load(tmp_path / f"result_{r}.pt", weights_only=False)
               for r in range(2)]
    # per-stage clipping would change the weights after the first step and
    # with them every later loss
    assert results[0][0] == pytest.approx(ref_losses, rel=1e-4), \
        (results[0][0], ref_losses)
    for losses, norms, local_norms in results:
        assert len(norms) == len(local_norms) == len(ref_norms)
        assert norms == pytest.approx(ref_norms, rel=1e-5), (norms, ref_norms)
        for n, ln in zip(norms, local_norms):
            assert ln < n * (1 - 1e-3), (ln, n)
    # the two stages' squares add up to the global value
    for t, n in enumerate(ref_norms):
        both = math.sqrt(results[0][2][t] ** 2 + results[1][2][t] ** 2)
        assert both == pytest.approx(n, rel=1e-5)
