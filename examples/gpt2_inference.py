#!/usr/bin/env python3
"""GPT-2 greedy decode demo (reference examples/gpt2_inference.cpp:19-127).

    python examples/gpt2_inference.py --model flash_gpt2_small \
        [--vocab vocab.bin] [--snapshot path] --prompt "Hello"

    python examples/gpt2_inference.py --bf16 --batch 8 --top-k 50 --top-p 0.95

``--batch N`` decodes N prompts together through ``generate_batch`` (one
hipGraph-captured step for all rows on GPU); ``--top-k`` / ``--top-p`` /
``--temperature`` / ``--seed`` switch it from greedy to on-device sampling.
``--draft MODEL --draft-k K`` decodes greedily through
``generate_speculative``: MODEL drafts K tokens per round, ``--model``
verifies them in one forward (same tokens as the plain greedy decode).

Without a vocab/snapshot this runs with random weights and raw token ids —
the compute path (embedding -> N gpt blocks -> ln_f -> head, full-sequence
recompute per token, matching the reference's no-KV-cache loop).
"""

import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tnn_amd import models
from tnn_amd.data import Tokenizer
from tnn_amd.models.generate import (generate, generate_batch,
                                      generate_cached, generate_speculative)
from tnn_amd.nn.layer import cast_compute_dtype
from tnn_amd.utils.checkpoint import load_model


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--model", default="flash_gpt2_small")
    p.add_argument("--snapshot", default=None)
    p.add_argument("--vocab", default=None)
    p.add_argument("--prompt", default="Hello world")
    p.add_argument("--tokens", type=int, default=50)
    p.add_argument("--seq-len", type=int, default=512)
    p.add_argument("--bf16", action="store_true")
    p.add_argument("--kv-cache", action="store_true",
                   help="cached decode (the reference recomputes)")
    p.add_argument("--batch", type=int, default=0,
                   help="decode this many prompts together (generate_batch)")
    p.add_argument("--top-k", type=int, default=0)
    p.add_argument("--top-p", type=float, default=1.0)
    p.add_argument("--temperature", type=float, default=1.0)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--draft", default=None,
                   help="draft model for greedy speculative decode "
                        "(generate_speculative)")
    p.add_argument("--draft-k", type=int, default=4,
                   help="draft tokens per round, 1..15")
    args = p.parse_args()

    model = (load_model(args.snapshot) if args.snapshot
             else models.create_model(args.model))
    if args.bf16:
        cast_compute_dtype(model, torch.bfloat16)
    dev = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    model.to(dev)

    tok = Tokenizer().load(args.vocab) if args.vocab else None
    prompt_ids = tok.encode(args.prompt) if tok else list(range(10))

    sampled = (args.top_k > 0 or args.top_p < 1.0 or args.temperature != 1.0)
    if args.draft:
        if sampled:
            p.error("--draft is greedy only")
        draft = models.create_model(args.draft)
        if args.bf16:
            cast_compute_dtype(draft, torch.bfloat16)
        draft.to(dev)
        n = max(args.batch, 1)
        prompts = [prompt_ids + prompt_ids[:b % len(prompt_ids)]
                   for b in range(n)]
        t0 = time.perf_counter()
        outs, stats = generate_speculative(
            model, draft, prompts, max_new_tokens=args.tokens,
            k=args.draft_k, seq_len=args.seq_len, device=dev,
            eot_token=50256 if tok else None, return_stats=True)
        dt = time.perf_counter() - t0
        n_new = sum(len(o) - len(q) for o, q in zip(outs, prompts))
        acc, dr = sum(stats["accepted"]), sum(stats["drafted"])
        print(f"{n_new} tokens in {dt:.2f}s ({n_new / dt:.2f} tok/s aggregate "
              f"over {n} sequences, speculative k={args.draft_k}: "
              f"{stats['rounds']} rounds, {acc} of {dr} drafts accepted)")
        for o in outs:
            print(tok.decode(o) if tok else o)
        return
    if args.batch > 0 or sampled:
        # the same prompt with a ragged tail of extra tokens per row
        n = max(args.batch, 1)
        prompts = [prompt_ids + prompt_ids[:b % len(prompt_ids)]
                   for b in range(n)]
        t0 = time.perf_counter()
        outs = generate_batch(model, prompts, max_new_tokens=args.tokens,
                              seq_len=args.seq_len, device=dev,
                              eot_token=50256 if tok else None,
                              greedy=not sampled,
                              temperature=args.temperature, top_k=args.top_k,
                              top_p=args.top_p, seed=args.seed)
        dt = time.perf_counter() - t0
        n_new = sum(len(o) - len(q) for o, q in zip(outs, prompts))
        print(f"{n_new} tokens in {dt:.2f}s ({n_new / dt:.2f} tok/s aggregate "
              f"over {n} sequences, {'sampled' if sampled else 'greedy'})")
        for o in outs:
            print(tok.decode(o) if tok else o)
        return

    gen = generate_cached if args.kv_cache else generate
    t0 = time.perf_counter()
    out = gen(model, prompt_ids, max_new_tokens=args.tokens,
              seq_len=args.seq_len, device=dev,
              eot_token=50256 if tok else None)
    dt = time.perf_counter() - t0
    n_new = len(out) - len(prompt_ids)
    mode = "kv-cache" if args.kv_cache else "full-sequence recompute"
    print(f"{n_new} tokens in {dt:.2f}s ({n_new / dt:.2f} tok/s, {mode})")
    print(tok.decode(out) if tok else out)


if __name__ == "__main__":
    main()
