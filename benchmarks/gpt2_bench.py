"""GPT-2 benchmarks (BASELINE config 4: GPT-2-small inference on 1x MI355X,
plus a training-step throughput measurement).

    python benchmarks/gpt2_bench.py [--model flash_gpt2_small] [--train]
"""

import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tnn_amd import models
from tnn_amd.nn import CrossEntropyLoss, AdamW
from tnn_amd.nn.layer import cast_compute_dtype
from tnn_amd.models.generate import (BatchedDecoder, DecodeSession, generate,
                                      generate_batch, generate_cached,
                                      generate_graphed, generate_speculative)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--model", default="flash_gpt2_small")
    p.add_argument("--seq-len", type=int, default=512)
    p.add_argument("--batch", type=int, default=8)
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--decode-tokens", type=int, default=32)
    p.add_argument("--decode-batch", type=int, default=0,
                   help="also time generate_batch over this many ragged "
                        "prompts (greedy, one captured step for all rows)")
    p.add_argument("--second-turn", action="store_true",
                   help="time a second turn of 64 tokens onto 8 live "
                        "contexts of 768 (DecodeSession) against "
                        "generate_batch on the concatenated prompts; wants "
                        "--seq-len 1024")
    p.add_argument("--speculative", action="store_true",
                   help="time greedy speculative decode (generate_speculative"
                        ", --draft proposes --draft-k tokens per round) on 8 "
                        "prompts of 3/4 seq-len: the target's single-token "
                        "step, the verify step, the draft's time per round "
                        "and tokens per second against generate_batch")
    p.add_argument("--draft", default="flash_gpt2_small")
    p.add_argument("--draft-k", type=int, default=4)
    p.add_argument("--train", action="store_true", default=True)
    p.add_argument("--graph", action="store_true",
                   help="also time the hipGraph-captured whole train step")
    p.add_argument("--max-grad-norm", type=float, default=0.0,
                   help="global-norm gradient clipping threshold of the "
                        "train step (0 = off)")
    args = p.parse_args()

    dev = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    model = models.create_model(args.model)
    if dev.type == "cuda":
        cast_compute_dtype(model, torch.bfloat16)
    model.to(dev)

    # ---- training-step throughput (tokens/s) ----
    if args.train and args.steps > 0:
        model.train()
        crit = CrossEntropyLoss()
        opt = AdamW(model.parameters(), lr=1e-4,
                    max_grad_norm=args.max_grad_norm)
        x = torch.randint(0, 50257, (args.batch, args.seq_len), device=dev)
        y = torch.randint(0, 50257, (args.batch, args.seq_len), device=dev)

        def step():
            out = model(x)
            loss = crit(out, y)
            opt.zero_grad()
            loss.backward()
            opt.step()
            return loss

        # graph capture must see FRESH AccumulateGrad nodes (eager steps
        # first would pin them to the default stream and crash capture)
        if args.graph and dev.type == "cuda":
            from tnn_amd.utils.graphstep import GraphedTrainStep
            gstep = GraphedTrainStep(model, crit, opt, x, y)
            for _ in range(3):
                gstep()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                gloss = gstep()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            toks = args.batch * args.seq_len * args.steps
            print(f"train[hipGraph]: {args.model} bs={args.batch} "
                  f"seq={args.seq_len}: {toks / dt:,.0f} tok/s "
                  f"({dt / args.steps * 1e3:.1f} ms/step, "
                  f"loss {gloss.item():.3f})")
            gstep.sync_step_count()
            opt._step_dev = None  # eager steps resume host step counting
            opt._lr_dev = None
            del gstep

        for _ in range(3):
            step()
        torch.cuda.synchronize() if dev.type == "cuda" else None
        t0 = time.perf_counter()
        for _ in range(args.steps):
            loss = step()
        torch.cuda.synchronize() if dev.type == "cuda" else None
        dt = time.perf_counter() - t0
        toks = args.batch * args.seq_len * args.steps
        print(f"train: {args.model} bs={args.batch} seq={args.seq_len}: "
              f"{toks / dt:,.0f} tok/s ({dt / args.steps * 1e3:.1f} ms/step, "
              f"loss {loss.item():.3f})")
        if args.max_grad_norm > 0:
            print(f"clip: max_grad_norm={args.max_grad_norm} last grad norm "
                  f"{opt.last_grad_norm.item():.3f}, skipped steps "
                  f"{opt.skipped_steps()}")



    # ---- greedy decode (reference gpt2_inference loop) ----
    # note: at batch 1 and short sequences decode is kernel-launch-bound on
    # a 2.5PF GPU, so the full-recompute loop (one big batch of launches)
    # can beat the eager KV cache (many tiny launches); the hipGraph path
    # captures the whole per-token step into one graph launch.
    model.eval()
    for name, fn in [("recompute (reference parity)", generate),
                     ("kv-cache", generate_cached),
                     ("hipGraph", generate_graphed)]:
        t0 = time.perf_counter()
        out = fn(model, list(range(16)), max_new_tokens=args.decode_tokens,
                 seq_len=args.seq_len, device=dev, eot_token=None)
        dt = time.perf_counter() - t0
        n = len(out) - 16
        print(f"decode [{name}]: {n} tokens in {dt:.2f}s = {n / dt:.2f} tok/s")
    if args.decode_batch > 0:
        prompts = [list(range(b, b + 9 + (7 * b) % 16))
                   for b in range(args.decode_batch)]
        for i in range(2):   # the second call is the steady-state figure
            t0 = time.perf_counter()
            outs = generate_batch(model, prompts,
                                  max_new_tokens=args.decode_tokens,
                                  seq_len=args.seq_len, device=dev,
                                  eot_token=None)
            dt = time.perf_counter() - t0
        n = sum(len(o) - len(q) for o, q in zip(outs, prompts))
        print(f"decode [batched x{args.decode_batch}]: {n} tokens in "
              f"{dt:.2f}s = {n / dt:.2f} tok/s aggregate, "
              f"{n / dt / args.decode_batch:.2f} tok/s per sequence")
    if args.second_turn:
        second_turn(model, dev, args.seq_len, args.decode_tokens)
    if args.speculative:
        draft = models.create_model(args.draft)
        if dev.type == "cuda":
            cast_compute_dtype(draft, torch.bfloat16)
        draft.to(dev).eval()
        speculative(model, draft, args.model, args.draft, dev, args.seq_len,
                    args.decode_tokens, args.draft_k)


def second_turn(model, dev, seq_len, n_tokens, rows=8, ctx_len=768, turn=64):
    """Second user turn onto live contexts: DecodeSession.generate (extend
    over the cached prefix) against generate_batch (close + full
    re-prefill of context + turn). Time to first token is a call with
    max_new_tokens=1. The routes alternate; the last of 3 rounds counts."""
    g = torch.Generator().manual_seed(0)
    ctx = [torch.randint(0, 50257, (ctx_len,), generator=g).tolist()
           for _ in range(rows)]
    new = [torch.randint(0, 50257, (turn,), generator=g).tolist()
           for _ in range(rows)]

    def sync():
        if dev.type == "cuda":
            torch.cuda.synchronize()

    def timed(fn):
        sync()
        t0 = time.perf_counter()
        out = fn()
        sync()
        return time.perf_counter() - t0, out

    sess = DecodeSession(model, rows, seq_len=seq_len, device=dev)
    try:
        sess.generate(ctx, max_new_tokens=0, eot_token=None)   # first turn
        res = {}
        for _ in range(3):
            for n, tag in ((1, "first token"), (n_tokens, "total")):
                sess.rewind([ctx_len] * rows)
                res["session", tag] = timed(lambda: sess.generate(
                    new, max_new_tokens=n, eot_token=None))
                res["batch", tag] = timed(lambda: generate_batch(
                    model, [c + t for c, t in zip(ctx, new)],
                    max_new_tokens=n, seq_len=seq_len, device=dev,
                    eot_token=None))
                # generate_batch closed the model's caches: reopen and
                # refill the session outside the timed region
                sess.close()
                sess = DecodeSession(model, rows, seq_len=seq_len, device=dev)
                sess.generate(ctx, max_new_tokens=0, eot_token=None)
        for tag in ("first token", "total"):
            print(f"second turn [{rows} x {ctx_len}+{turn}, {n_tokens} new] "
                  f"{tag}: DecodeSession {res['session', tag][0] * 1e3:.1f} ms"
                  f" | generate_batch {res['batch', tag][0] * 1e3:.1f} ms")
    finally:
        sess.close()


def speculative(model, draft, mname, dname, dev, seq_len, n_tokens, k,
                rows=8, iters=30):
    """Greedy speculative decode: step times of its three parts on live
    caches of ``rows`` contexts of 3/4 seq_len, then whole calls against
    generate_batch. Single-token steps are timed as captured graphs (what
    both loops replay), the verify step eagerly (what the loop runs); every
    window is ``iters`` calls ending in a synchronise, after a warm-up."""
    from tnn_amd.ops import sample_logits
    ctx_len = seq_len * 3 // 4
    g = torch.Generator().manual_seed(0)
    prompts = [torch.randint(0, 50257, (ctx_len,), generator=g).tolist()
               for _ in range(rows)]

    def sync():
        if dev.type == "cuda":
            torch.cuda.synchronize()

    def window(fn, n=iters, warm=5):
        for _ in range(warm):
            fn()
        sync()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        sync()
        return (time.perf_counter() - t0) / n

    def step_time(m, per_call):
        """one single-token step of the decode loops, graph-replayed
        ``per_call`` times from the same positions"""
        dec = BatchedDecoder(m, seq_len, dev)
        try:
            dec.prefill(prompts)
            tok = torch.zeros(rows, 1, dtype=torch.int64, device=dev)
            saved = dec.pos.clone()

            def step():
                nxt = sample_logits(dec.forward_token(tok), temperature=0)
                tok.copy_(nxt.reshape(rows, 1))
                dec.advance()

            run = step
            if dev.type == "cuda":
                stream = torch.cuda.Stream()
                stream.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(stream):
                    for _ in range(2):
                        step()
                torch.cuda.current_stream().wait_stream(stream)
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    step()
                run = graph.replay

            def call():
                dec.pos.copy_(saved)
                for _ in range(per_call):
                    run()
            return window(call)
        finally:
            dec.close()

    def verify_time(split):
        dec = BatchedDecoder(model, seq_len, dev)
        try:
            dec.prefill(prompts)
            x = torch.randint(0, 50257, (rows, k + 1), generator=g).to(dev)
            n = torch.full((rows,), k + 1, dtype=torch.int64, device=dev)
            saved = dec.pos.clone()

            def call():
                dec.pos.copy_(saved)
                if split:
                    dec._verify(x, n)
                else:
                    lg = dec._extend_logits(x, n, 0)
                    sample_logits(lg.reshape(rows * (k + 1), -1),
                                  temperature=0)
            return window(call)
        finally:
            dec.close()

    with torch.no_grad():
        t_step = step_time(model, 1)
        t_draft = step_time(draft, k + 1)
        t_ver, t_ver0 = verify_time(True), verify_time(False)
    heads = {a.num_heads for a in model.modules() if hasattr(a, "num_heads")}
    print(f"speculative [{mname} <- {dname}, k={k}, {rows} x {ctx_len}]: "
          f"target step {t_step * 1e3:.3f} ms | verify T={k + 1} "
          f"{t_ver * 1e3:.3f} ms (unsplit attention {t_ver0 * 1e3:.3f} ms, "
          f"heads {sorted(heads)}) | draft round ({k + 1} steps) "
          f"{t_draft * 1e3:.3f} ms")
    round_t = t_draft + t_ver
    print(f"speculative: round / step = {round_t / t_step:.2f}, verify / "
          f"step = {t_ver / t_step:.2f}, draft step / step = "
          f"{t_draft / (k + 1) / t_step:.2f}; break-even at "
          f"{round_t / t_step - 1:.2f} accepted drafts per round of {k} "
          f"(device time only)")
    for name, fn in (
            ("generate_batch", lambda: generate_batch(
                model, prompts, max_new_tokens=n_tokens, seq_len=seq_len,
                device=dev, eot_token=None)),
            ("generate_speculative", lambda: generate_speculative(
                model, draft, prompts, max_new_tokens=n_tokens, k=k,
                seq_len=seq_len, device=dev, eot_token=None,
                return_stats=True))):
        for _ in range(2):   # the second call is the steady-state figure
            sync()
            t0 = time.perf_counter()
            out = fn()
            sync()
            dt = time.perf_counter() - t0
        stats = None
        if isinstance(out, tuple):
            out, stats = out
        n = sum(len(o) - len(q) for o, q in zip(out, prompts))
        line = (f"decode [{name} x{rows}]: {n} tokens in {dt:.3f}s = "
                f"{n / dt:.1f} tok/s")
        if stats:
            acc, dr = sum(stats["accepted"]), sum(stats["drafted"])
            line += (f"; {stats['rounds']} rounds, accepted {acc} of {dr} "
                     f"drafts ({acc / max(dr, 1):.3f})")
        print(line)


if __name__ == "__main__":
    main()
