"""Gradient clipping under the data-parallel engine (gloo, 2 ranks): after
the bucketed all-reduce every rank holds the full-batch gradient, so the
local norm is the global one and no norm reduction is installed. Clipped
SGD on 2 ranks must match clipped single-process full-batch SGD, and both
ranks must report the full-batch norm."""

import os

import pytest
import torch
import torch.multiprocessing as mp

from tnn_amd.nn import LayerBuilder, CrossEntropyLoss, SGD

# well below this model's gradient norm: clips every step (asserted on the
# reference norms)
MAX_NORM = 0.05
STEPS = 3


def _model(seed=3):
    torch.manual_seed(seed)
    # BN-free: per-shard batch statistics would break exact parity
    return (LayerBuilder((6, 6, 2))
            .conv2d(4, 3, 3, 1, 1, 1, 1, True, "c1")
            .activation("relu", "r1")
            .flatten()
            .dense(3, True, "fc")
            .build("ddp_clip_test"))


def _data(seed=11):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(16, 6, 6, 2, generator=g)
    y = torch.randint(0, 3, (16,), generator=g)
    return x, y


def _ddp_worker(rank, world, tmpdir):
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method=f"file://{tmpdir}/pg",
                            rank=rank, world_size=world)
    from tnn_amd.parallel import Communicator, DataParallelEngine
    comm = Communicator()
    model = _model(seed=3 + rank)  # engine broadcasts rank 0's weights
    engine = DataParallelEngine(model, comm, bucket_bytes=256)
    crit = CrossEntropyLoss()
    opt = SGD(model.parameters(), lr=0.5, max_grad_norm=MAX_NORM)
    assert opt.norm_reduce is None
    x, y = _data()
    shard_x = x.chunk(world)[rank]
    shard_y = y.chunk(world)[rank]
    norms = []
    for _ in range(STEPS):
        loss = crit(model(shard_x), shard_y)
        opt.zero_grad()
        engine.train_step(loss, opt)
        norms.append(opt.last_grad_norm.item())
    torch.save(({k: v.clone() for k, v in model.state_dict().items()}, norms),
               os.path.join(tmpdir, f"sd_{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_ddp_clipping_matches_full_batch(tmp_path):
    model = _model(seed=3)
    crit = CrossEntropyLoss()
    opt = SGD(model.parameters(), lr=0.5, max_grad_norm=MAX_NORM)
    x, y = _data()
    ref_norms = []
    for _ in range(STEPS):
        loss = crit(model(x), y)
        opt.zero_grad()
        loss.backward()
        opt.step()
        ref_norms.append(opt.last_grad_norm.item())
    assert all(n > MAX_NORM for n in ref_norms), ref_norms

    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_ddp_worker, args=(r, 2, str(tmp_path)))
             for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=180)
        assert p.exitcode == 0
    sd0, norms0 = torch.load(tmp_path / "sd_0.pt", weights_only=False)
    sd1, norms1 = torch.load(tmp_path / "sd_1.pt", weights_only=False)
    # same bound on the norm as the pipeline test; weights at the bounds of
    # test_ddp_matches_full_batch
    assert norms0 == pytest.approx(ref_norms, rel=1e-5)
    assert norms1 == pytest.approx(ref_norms, rel=1e-5)
    ref = model.state_dict()
    for k in ref:
        assert torch.allclose(sd0[k], sd1[k], atol=1e-6), k
        assert torch.allclose(sd0[k], ref[k], atol=1e-4), \
            (k, (sd0[k] - ref[k]).abs().max())
