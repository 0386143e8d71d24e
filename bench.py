"""Flagship benchmark: WRN-16-8 pipeline-parallel training throughput
(images/sec, whole node) on synthetic 32x32x3 data — BASELINE.json's
headline metric. Reference numbers: ~1,900-2,530 img/s for the same model
at batch 256 on 2 consumer GPUs over RoCE.

Single process:   python bench.py --gpus 1 --steps 30 --warmup 10
Multi-GPU (driver): python -m torch.distributed.run --nnodes=1
    --nproc-per-node N --master-addr 127.0.0.1 bench.py --gpus N ...

Weak scaling: global batch = 256 * N (per-GPU work constant as the model
is split N ways while the batch grows N ways).

A plain run sets up, warms up, times ``--steps`` steps and prints one JSON
result line. ``--dump-outputs DIR`` additionally writes what the last timed
step returned as ``DIR/<name>.npy``; weights, data and dropout salts are
seeded, so two builds run with the same arguments see identical inputs.
``--full`` is reserved for measurements beyond the headline figure.
"""

import argparse
import json
import os
import random
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

BASELINE_IMG_S = 2530.0  # top of the reference band (BASELINE.md per-batch)
SEED = 1234


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=int(os.environ.get("WORLD_SIZE", 1)))
    p.add_argument("--steps", type=int, default=30)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--model", default="cifar100_wrn16_8")
    p.add_argument("--batch-per-gpu", type=int, default=256)
    p.add_argument("--microbatch", type=int, default=32,
                   help="micro-batch size for the 1F1B schedule: 8 "
                        "microbatches per pipeline stage (bubble fraction "
                        "(N-1)/(8N+N-1)); conv M stays >=32k rows so "
                        "per-kernel efficiency holds")
    p.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    p.add_argument("--lr", type=float, default=1e-3)
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps, write what the last timed "
                        "step returned (its loss) as DIR/<name>.npy in "
                        "float32")
    p.add_argument("--full", action="store_true",
                   help="also run the measurements that are not needed for "
                        "the headline figure (none at present: a plain run "
                        "already does only setup, warmup, the timed steps "
                        "and the result line)")
    return p.parse_args()


def dump_outputs(out_dir, last):
    """Write what the last timed step returned as float32 ``.npy`` files.

    ``last`` is the timed callable's return value: the device loss tensor
    of the graphed step (``loss.npy``), or train_batch's stats dict
    (``loss.npy``, ``accuracy.npy``). A few floats, far below any size cap.

    The trained parameters are deliberately not written. Conv biases that
    feed a batch norm have a mathematically zero gradient, so theirs is pure
    accumulation-order noise, which Adam's normalisation turns into +-lr
    updates: measured on MI355X, two runs of the same build differ there by
    more than the values themselves after 4 steps, while the loss agrees to
    3e-5 relative (3e-3 after 43 steps). They cannot tell two builds apart.
    """
    if isinstance(last, dict):
        arrays = {k: np.asarray([v], dtype=np.float32)
                  for k, v in last.items()}
    else:
        arrays = {"loss": last.detach().float().cpu().numpy()
                  .reshape(-1).astype(np.float32)}
    os.makedirs(out_dir, exist_ok=True)
    for k, a in arrays.items():
        np.save(os.path.join(out_dir, k + ".npy"), a)


def main():
    args = parse_args()
    # weights come from torch's global RNG and graph-captured dropout salts
    # from python's: seed both so every run starts from identical inputs
    random.seed(SEED)
    np.random.seed(SEED)
    torch.manual_seed(SEED)
    from tnn_amd import models
    from tnn_amd.nn import CrossEntropyLoss
    from tnn_amd.parallel import init_distributed, PipelineEngine

    have_gpu = torch.cuda.is_available()
    device = torch.device("cuda" if have_gpu else "cpu")
    dtype = torch.bfloat16 if (args.dtype == "bf16" and have_gpu) else torch.float32

    comm = init_distributed()
    world = comm.world_size
    rank = comm.rank
    assert world == args.gpus or args.gpus == 1, \
        f"launched with WORLD_SIZE={world} but --gpus {args.gpus}"

    global_batch = args.batch_per_gpu * world
    num_micro = max(1, global_batch // args.microbatch) if world > 1 else 1

    model = models.create_model(args.model) if rank == 0 else None
    shapes = {
        "mnist_cnn": ((28, 28, 1), 10),
        "cifar100_wrn16_8": ((32, 32, 3), 100),
        "cifar10_resnet9": ((32, 32, 3), 10),
        "cifar10_vgg": ((32, 32, 3), 10),
        "cifar100_resnet18": ((32, 32, 3), 100),
        "tiny_imagenet_wrn16_8": ((64, 64, 3), 200),
        "tiny_imagenet_resnet18": ((64, 64, 3), 200),
        "tiny_imagenet_resnet50": ((64, 64, 3), 200),
        "tiny_imagenet_vit": ((64, 64, 3), 200),
        "tiny_imagenet_flash_vit": ((64, 64, 3), 200),
        "imagenet_resnet50": ((224, 224, 3), 1000),
    }
    in_shape, num_classes = shapes.get(args.model, ((32, 32, 3), 100))

    engine = PipelineEngine(
        model, comm, input_shape=in_shape, num_microbatches=num_micro,
        criterion=CrossEntropyLoss(),
        optimizer_config={"type": "adamw", "lr": args.lr},
        device=device, io_dtype=dtype)

    # fixed synthetic batch, random-init weights (no network for datasets)
    g = torch.Generator().manual_seed(SEED)
    x = torch.randn(global_batch, *in_shape, generator=g).to(device)
    y = torch.randint(0, num_classes, (global_batch,), generator=g).to(device)

    # single-GPU: capture the whole train step (grad zero + fwd + loss +
    # bwd + fused optimizer) as ONE hipGraph and replay it — identical
    # kernels, no per-launch host dispatch gaps. Disable: TNN_BENCH_GRAPH=0.
    graphed = (world == 1 and have_gpu
               and os.environ.get("TNN_BENCH_GRAPH", "1") != "0")
    if graphed:
        from tnn_amd.utils.graphstep import GraphedTrainStep
        try:
            gstep = GraphedTrainStep(engine.stage, engine.criterion,
                                     engine.optimizer, x, y)
            run_step = gstep
        except Exception as e:  # capture failure: measure eager instead
            print(f"[bench] graph capture failed ({e}); eager fallback",
                  file=sys.stderr)
            graphed = False
            run_step = lambda: engine.train_batch(x, y)  # noqa: E731
    else:
        run_step = lambda: engine.train_batch(x, y)  # noqa: E731

    for _ in range(args.warmup):
        run_step()

    comm.barrier()
    if have_gpu:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    last = None
    for _ in range(args.steps):
        last = run_step()
    comm.barrier()
    if have_gpu:
        torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0

    # max over ranks
    t = torch.tensor([elapsed], dtype=torch.float64)
    if world > 1:
        import torch.distributed as dist
        tt = t.to(device) if comm.backend == "nccl" else t
        dist.all_reduce(tt, dist.ReduceOp.MAX)
        elapsed = float(tt.cpu().item())

    if args.dump_outputs and args.steps > 0 and rank == world - 1:
        dump_outputs(args.dump_outputs, last)

    if rank == 0:
        value = global_batch * args.steps / elapsed
        print(json.dumps({
            "metric": "images/sec (whole node) WRN-16-8 on 32x32x3, "
                      "pipeline-parallel",
            "value": round(value, 1),
            "unit": "img/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": round(value / BASELINE_IMG_S, 2),
            "dtype": "bf16" if dtype == torch.bfloat16 else "fp32",
            "data": "synthetic",
            "config": {
                "model": args.model,
                "global_batch": global_batch,
                "input": "x".join(map(str, in_shape)),
                "microbatches": num_micro,
                "graphed_step": graphed,
                "parallelism": f"pp{world}" if world > 1 else "single",
            },
        }))


if __name__ == "__main__":
    main()
