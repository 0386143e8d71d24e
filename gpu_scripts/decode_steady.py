"""Steady-state decode rate: second and later calls after warm capture
infrastructure (the serving loop's regime).

    python gpu_scripts/decode_steady.py                  # generate_graphed, B=1
    python gpu_scripts/decode_steady.py --batch 1,4,8,16 [--top-k 50 --top-p 0.95]

With --batch the prompts go through generate_batch (one captured step over
all rows); a sampled run is added when --top-k / --top-p / --temperature
ask for one. Prints aggregate and per-sequence tok/s and ms per step."""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from tnn_amd import models
from tnn_amd.nn.layer import cast_compute_dtype
from tnn_amd.models.generate import generate_batch, generate_graphed

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="flash_gpt2_small")
ap.add_argument("--batch", default=None,
                help="comma-separated batch sizes for generate_batch")
ap.add_argument("--new-tokens", type=int, default=256)
ap.add_argument("--calls", type=int, default=3)
ap.add_argument("--top-k", type=int, default=0)
ap.add_argument("--top-p", type=float, default=1.0)
ap.add_argument("--temperature", type=float, default=1.0)
ap.add_argument("--seed", type=int, default=0)
args = ap.parse_args()

m = models.create_model(args.model)
cast_compute_dtype(m, torch.bfloat16)
m.to("cuda").eval()
N = args.new_tokens


def run(label, fn, nseq):
    for i in range(args.calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n_new = fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print(f"{label} call {i}: {n_new} tokens in {dt:.3f}s = "
              f"{n_new / dt:.0f} tok/s aggregate, {n_new / dt / nseq:.0f} "
              f"tok/s per sequence, {dt / N * 1e3:.3f} ms/step", flush=True)


def graphed():
    out = generate_graphed(m, list(range(16)), max_new_tokens=N,
                           seq_len=1024, eot_token=None)
    return len(out) - 16


run("generate_graphed B=1", graphed, 1)
if args.batch:
    sampled = args.top_k > 0 or args.top_p < 1.0 or args.temperature != 1.0
    for B in (int(b) for b in args.batch.split(",")):
        # ragged prompts of 9..24 tokens
        prompts = [list(range(b, b + 9 + (7 * b) % 16)) for b in range(B)]

        def batch(greedy):
            outs = generate_batch(m, prompts, max_new_tokens=N, seq_len=1024,
                                  eot_token=None, greedy=greedy,
                                  temperature=args.temperature,
                                  top_k=args.top_k, top_p=args.top_p,
                                  seed=args.seed)
            return sum(len(o) - len(p) for o, p in zip(outs, prompts))

        run(f"generate_batch B={B} greedy", lambda: batch(True), B)
        if sampled:
            run(f"generate_batch B={B} top_k={args.top_k} top_p={args.top_p}",
                lambda: batch(False), B)
