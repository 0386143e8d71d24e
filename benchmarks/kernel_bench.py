"""Kernel micro-benchmarks (reference benchmarks/{gemm,conv2d,dense,
batchnorm,...}_benchmark.cpp analog).

    python benchmarks/kernel_bench.py [op ...]   # default: all

Prints one line per case: op, shape, ms, TFLOP/s (or GB/s for memory ops).
"""

import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tnn_amd import _C  # noqa: E402

ext = _C.ext() if torch.cuda.is_available() else None
DEV = "cuda"


def timeit(fn, iters=50, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def report(name, shape, secs, flops=None, bytes_=None):
    extra = ""
    if flops:
        extra = f"{flops / secs / 1e12:8.2f} TF/s"
    if bytes_:
        extra += f"{bytes_ / secs / 1e12:8.2f} TB/s"
    print(f"{name:18s} {shape:42s} {secs * 1e3:8.3f} ms {extra}")


def bench_gemm(dtype=torch.bfloat16):
    for M, N, K in [(4096, 4096, 4096), (65536, 128, 1152), (16384, 512, 4608),
                    (8192, 768, 768), (256, 100, 512)]:
        a = torch.randn(M, K, dtype=dtype, device=DEV)
        b = torch.randn(K, N, dtype=dtype, device=DEV)
        secs = timeit(lambda: ext.gemm(a, b, None, 0))
        report("gemm_nn", f"{M}x{N}x{K} {dtype}", secs, 2.0 * M * N * K)


def bench_conv(dtype=torch.bfloat16):
    cases = [
        ("g1 conv 128->128", 256, 32, 32, 128, 128, 3, 1, 1),
        ("g2 conv 256->256", 256, 16, 16, 256, 256, 3, 1, 1),
        ("g3 conv 512->512", 256, 8, 8, 512, 512, 3, 1, 1),
        ("stride2 128->256", 256, 32, 32, 128, 256, 3, 2, 1),
    ]
    for name, N, H, W, Ci, Co, KS, S, P in cases:
        x = torch.randn(N, H, W, Ci, dtype=dtype, device=DEV)
        w = torch.randn(KS, KS, Ci, Co, dtype=dtype, device=DEV) * 0.05
        OH = (H + 2 * P - KS) // S + 1
        dy = torch.randn(N, OH, OH, Co, dtype=dtype, device=DEV)
        fl = 2.0 * N * OH * OH * Co * KS * KS * Ci
        report(f"conv_fwd", f"{name} mb{N}", timeit(lambda: ext.conv2d_fwd(
            x, w, None, S, S, P, P, False)), fl)
        report(f"conv_dgrad", f"{name} mb{N}", timeit(lambda: ext.conv2d_dgrad(
            dy, w, H, W, S, S, P, P)), fl)
        report(f"conv_wgrad", f"{name} mb{N}", timeit(lambda: ext.conv2d_wgrad(
            x, dy, KS, KS, S, S, P, P, False)), fl)
        # weight + bias gradient: the fused binding vs the pair it replaces
        report(f"conv_wgrad+bias", f"{name} mb{N}", timeit(
            lambda: ext.conv2d_wgrad_bias(x, dy, KS, KS, S, S, P, P, False)),
            fl)
        dy2 = dy.reshape(-1, Co)
        report(f"conv_wgrad,colsum", f"{name} mb{N}", timeit(
            lambda: (ext.conv2d_wgrad(x, dy, KS, KS, S, S, P, P, False),
                     ext.colsum(dy2))), fl)


def bench_bn(dtype=torch.bfloat16):
    for C in [128, 512]:
        rows = 256 * 32 * 32 if C == 128 else 256 * 8 * 8
        x = torch.randn(rows // (8 * 8), 8, 8, C, dtype=dtype, device=DEV)
        g = torch.ones(C, device=DEV)
        b = torch.zeros(C, device=DEV)
        nbytes = x.numel() * x.element_size()
        secs = timeit(lambda: ext.bn_fwd_train(x, g, b, None, None, 0.1, 1e-5, True, 0.0, 0, None))
        report("bn_fwd_train", f"rows={rows} C={C} {dtype}", secs,
               bytes_=3 * nbytes)


def bench_colsum(dtype=torch.bfloat16):
    x = torch.randn(256 * 32 * 32, 128, dtype=dtype, device=DEV)
    secs = timeit(lambda: ext.colsum(x))
    report("colsum", f"{tuple(x.shape)} {dtype}", secs,
           bytes_=x.numel() * x.element_size())


def bench_ce(dtype=torch.bfloat16):
    logits = torch.randn(8192, 50257, dtype=dtype, device=DEV)
    t = torch.randint(0, 50257, (8192,), device=DEV)
    secs = timeit(lambda: ext.ce_fwd(logits, t))
    report("ce_fwd", "8192x50257", secs,
           bytes_=logits.numel() * logits.element_size())


def bench_attn():
    for B, H, S, D, causal in [(8, 12, 512, 64, True), (8, 12, 1024, 64, True),
                               (2, 16, 2048, 128, False)]:
        q = torch.randn(B, H, S, D, dtype=torch.bfloat16, device=DEV)
        k = torch.randn_like(q)
        v = torch.randn_like(q)
        fl = 4.0 * B * H * S * S * D * (0.5 if causal else 1.0)
        secs = timeit(lambda: ext.attn_fwd(q, k, v, causal))
        report("attn_fwd", f"B{B} H{H} S{S} D{D} causal={causal}", secs, fl)
        o, lse = ext.attn_fwd(q, k, v, causal)
        do = torch.randn_like(q)
        secs = timeit(lambda: ext.attn_bwd(q, k, v, o, do, lse, causal),
                      iters=20)
        report("attn_bwd", f"B{B} H{H} S{S} D{D} causal={causal}", secs,
               2.5 * fl)


def bench_attn_extend():
    """Extend attention (T new rows per sequence at prefix pos) against the
    cached-prefill route it replaces, sdpa_materialized over the live
    prefix with qoff = pos, and -- at pos = 0, where the work is the same
    -- causal attn_fwd at S = T. The routes of a shape are timed in turn,
    twice; the better round is reported. FLOPs count visible keys only."""
    from tnn_amd import ops
    cap = 1024
    for B, H, D in [(8, 12, 64), (8, 20, 64), (8, 8, 128)]:
        kc = torch.randn(B, H, cap, D, dtype=torch.bfloat16, device=DEV)
        vc = torch.randn_like(kc)
        for pos, T in [(0, 128), (0, 512), (0, 1024), (512, 512), (960, 64),
                       (1016, 8)]:
            qkv = torch.randn(B, T, 3 * H * D, dtype=torch.bfloat16,
                              device=DEV)
            q = qkv[..., :H * D].view(B, T, H, D).transpose(1, 2)
            pos_t = torch.full((B,), pos, dtype=torch.int64, device=DEV)
            kl, vl = kc[:, :, :pos + T], vc[:, :, :pos + T]
            routes = {
                "attn_extend": lambda: ext.attn_extend(q, kc, vc, pos_t, None,
                                                       D ** -0.5),
                "sdpa_materialized": lambda: ops.sdpa_materialized(
                    q, kl, vl, causal=True, qoff=pos)}
            if pos == 0:
                qd, kd, vd = q.contiguous(), kl.contiguous(), vl.contiguous()
                routes["attn_fwd"] = lambda: ext.attn_fwd(qd, kd, vd, True)
            fl = 4.0 * B * H * D * (T * pos + T * (T + 1) / 2)
            best = {}
            with torch.no_grad():
                for _ in range(2):
                    for name, fn in routes.items():
                        secs = timeit(fn)
                        best[name] = min(secs, best.get(name, secs))
            for name, secs in best.items():
                report(name, f"B{B} H{H} D{D} pos{pos} T{T}", secs, fl)
        # split-KV rows (verify-step shapes, T <= 16): kv_splits = 0 is the
        # unsplit kernel above; "auto" names what attn_extend_splits picks
        for pos, T in [(1016, 8), (1008, 16), (960, 16), (512, 8), (64, 8),
                       (0, 8)]:
            qkv = torch.randn(B, T, 3 * H * D, dtype=torch.bfloat16,
                              device=DEV)
            q = qkv[..., :H * D].view(B, T, H, D).transpose(1, 2)
            pos_t = torch.full((B,), pos, dtype=torch.int64, device=DEV)
            routes = {
                ns: (lambda ns=ns: ext.attn_extend(q, kc, vc, pos_t, None,
                                                   D ** -0.5, ns))
                for ns in (0, 1, 2, 4, 8, 16)}
            fl = 4.0 * B * H * D * (T * pos + T * (T + 1) / 2)
            best = {}
            with torch.no_grad():
                for _ in range(2):
                    for ns, fn in routes.items():
                        secs = timeit(fn)
                        best[ns] = min(secs, best.get(ns, secs))
            auto = ext.attn_extend_splits(B * H, cap, T)
            for ns, secs in best.items():
                report(f"attn_extend ns{ns}" + ("*" if ns == auto else ""),
                       f"B{B} H{H} D{D} pos{pos} T{T}", secs, fl)
        print(f"(* = automatic split count for B*H={B * H} cap={cap})")


def bench_attn_extend_splits():
    """Split counts of the split-KV extend kernel away from the B=8 head
    configurations of bench_attn_extend: few and many (b, h) rows, a short
    and a long cache. What the table above attn_ext_splits rests on; same
    protocol (routes in turn, twice, better round)."""
    D = 64
    for B, H, cap in [(1, 12, 1024), (1, 20, 1024), (4, 8, 1024),
                      (4, 2, 320), (16, 12, 1024), (16, 20, 1024),
                      (8, 12, 4096)]:
        kc = torch.randn(B, H, cap, D, dtype=torch.bfloat16, device=DEV)
        vc = torch.randn_like(kc)
        for pos, T in [(cap - 8, 8), (cap // 2, 8), (cap - 16, 5)]:
            q = torch.randn(B, H, T, D, dtype=torch.bfloat16, device=DEV)
            pos_t = torch.full((B,), pos, dtype=torch.int64, device=DEV)
            best = {}
            for _ in range(2):
                for ns in (0, 2, 3, 4, 6, 8, 16):
                    secs = timeit(lambda: ext.attn_extend(
                        q, kc, vc, pos_t, None, D ** -0.5, ns))
                    best[ns] = min(secs, best.get(ns, secs))
            auto = ext.attn_extend_splits(B * H, cap, T)
            print(f"attn_extend BH{B * H} cap{cap} pos{pos} T{T} auto={auto} us:"
                  + "".join(f" ns{n}={s * 1e6:.1f}" for n, s in best.items()))


def bench_bmm():
    # materialized-scores attention shapes (per-head batched QK^T)
    for BH, S, D in [(96, 512, 64), (32, 2048, 128)]:
        a = torch.randn(BH, S, D, dtype=torch.bfloat16, device=DEV)
        b = torch.randn(BH, S, D, dtype=torch.bfloat16, device=DEV)
        fl = 2.0 * BH * S * S * D
        secs = timeit(lambda: ext.bmm(a, b.transpose(-1, -2)))
        report("bmm_nt", f"BH{BH} S{S} D{D} (QK^T)", secs, fl)


def bench_softmax():
    from tnn_amd import ops
    for BH, S in [(96, 512), (32, 2048)]:
        x = torch.randn(BH, S, S, dtype=torch.bfloat16, device=DEV)
        by = 2 * x.numel() * 2
        secs = timeit(lambda: ext.smax_fwd(x, S, 0, 0.125, True))
        report("smax_fwd", f"BH{BH} S{S} causal", secs, bytes_=by)


def bench_ln():
    for R, C in [(4096, 768), (8192, 1024)]:
        x = torch.randn(R, C, dtype=torch.bfloat16, device=DEV)
        g = torch.randn(C, device=DEV)
        b = torch.randn(C, device=DEV)
        by = 2 * x.numel() * 2
        secs = timeit(lambda: ext.ln_fwd(x, g, b, 1e-5))
        report("ln_fwd", f"{R}x{C}", secs, bytes_=by)


def bench_gn():
    for N, HW, C, G in [(256, 64, 256, 32)]:
        x = torch.randn(N, HW, C, dtype=torch.bfloat16, device=DEV)
        g = torch.randn(C, device=DEV)
        b = torch.randn(C, device=DEV)
        by = 2 * x.numel() * 2
        secs = timeit(lambda: ext.gn_fwd(x, g, b, G, 1e-5))
        report("gn_fwd", f"N{N} HW{HW} C{C} G{G}", secs, bytes_=by)


def bench_decode():
    from tnn_amd import ops
    BH, cap, D = 12, 1024, 64
    q = torch.randn(BH, D, dtype=torch.bfloat16, device=DEV)
    kc = torch.randn(BH, cap, D, dtype=torch.bfloat16, device=DEV)
    vc = torch.randn_like(kc)
    secs = timeit(lambda: ops.attention_decode(q, kc, vc, None, cap,
                                               D ** -0.5))
    report("attn_decode", f"BH{BH} cap{cap} D{D}", secs,
           bytes_=2 * BH * cap * D * 2)


def bench_skinny(dtype=torch.bfloat16):
    """Batched-decode linears: the skinny route (ext.gemm_skinny) against
    the general path the same rows take with TNN_SKINNY=0 (ext.gemm),
    alternated in one session, next to the M=1 GEMV of the same weights.
    Each call streams a different copy of the weights (a ring larger than
    the caches would be the decode loop's regime; the ring here is capped
    at 64 copies / 512 MB)."""
    es = torch.empty(0, dtype=dtype).element_size()
    for K, N in [(768, 2304), (768, 3072), (3072, 768), (768, 50257)]:
        wbytes = K * N * es
        ncopy = max(2, min(64, (512 << 20) // wbytes))
        ws = [torch.randn(K, N, dtype=dtype, device=DEV) * 0.05
              for _ in range(ncopy)]
        b = torch.randn(N, dtype=dtype, device=DEV)
        it = [0]

        def nxt():
            it[0] = (it[0] + 1) % ncopy
            return ws[it[0]]

        x1 = torch.randn(1, K, dtype=dtype, device=DEV)
        t1 = min(timeit(lambda: ext.gemm(x1, nxt(), b, 0), iters=100)
                 for _ in range(3))
        report("gemv_m1", f"M1 K{K} N{N}", t1, bytes_=wbytes)
        for M in (2, 4, 8, 16):
            x = torch.randn(M, K, dtype=dtype, device=DEV)
            ts, tg = [], []
            for _ in range(3):   # alternate the two routes
                ts.append(timeit(lambda: ext.gemm_skinny(x, nxt(), b, 0),
                                 iters=100))
                tg.append(timeit(lambda: ext.gemm(x, nxt(), b, 0),
                                 iters=100))
            report("gemm_skinny", f"M{M} K{K} N{N}", min(ts), bytes_=wbytes)
            report("gemm_general", f"M{M} K{K} N{N}", min(tg), bytes_=wbytes)
            print(f"{'':18s} skinny/M1 = {min(ts) / t1:.2f}x   "
                  f"general/skinny = {min(tg) / min(ts):.2f}x")
        del ws


def bench_sample():
    R, V = 16, 50257
    logits = (torch.randn(R, V, device=DEV) * 2).to(torch.bfloat16)
    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    for name, t, k, p in [("greedy", 0.0, 0, 1.0), ("temperature", 0.8, 0, 1.0),
                          ("top_k=50", 0.8, 50, 1.0), ("top_p=0.95", 0.8, 0, 0.95),
                          ("top_k=50 top_p=0.95", 0.8, 50, 0.95)]:
        secs = timeit(lambda: ext.sample_logits(logits, t, k, p, 0, step),
                      iters=200)
        report("sample_logits", f"R{R} V{V} {name}", secs,
               bytes_=logits.numel() * 2)
    secs = timeit(lambda: logits.argmax(-1), iters=200)
    report("torch argmax", f"R{R} V{V}", secs, bytes_=logits.numel() * 2)


def bench_gradnorm():
    """Global gradient norm (k_gradsq_mt + k_clip_fin) at the GPT-2-small
    gradient size: 124.4M elements split like the model's tensors (the
    embedding, 12 blocks of attention/MLP matrices, the small vectors)."""
    from tnn_amd.nn.optim import _GradNormWorkspace
    shapes = [(50257, 768), (1024, 768)]
    for _ in range(12):
        shapes += [(768, 2304), (2304,), (768, 768), (768,), (768, 3072),
                   (3072,), (3072, 768), (768,), (768,), (768,), (768,),
                   (768,)]
    shapes += [(768,), (768,)]
    for dtype in (torch.bfloat16, torch.float32):
        grads = [torch.randn(*s, device=DEV).to(dtype) for s in shapes]
        n = sum(g.numel() for g in grads)
        ws = _GradNormWorkspace()
        dev = grads[0].device
        # descriptors built once, as in a warmed-up optimizer step: the
        # timed call is the two launches
        recs = ws.loose_records(list(enumerate(grads)), dev)
        secs = timeit(lambda: ws.run(ext, recs, dev, 1.0, count_skips=False),
                      iters=200)
        nbytes = n * grads[0].element_size()
        shape = f"{len(grads)} tensors {n / 1e6:.1f}M {dtype}"
        print(f"{'grad_global_norm':18s} {shape:42s} {secs * 1e3:8.3f} ms "
              f"{nbytes / secs / 1e9:8.1f} GB/s")


ALL = {"gemm": bench_gemm, "conv": bench_conv, "bn": bench_bn,
       "colsum": bench_colsum, "ce": bench_ce, "attn": bench_attn,
       "attn_extend": bench_attn_extend,
       "attn_extend_splits": bench_attn_extend_splits, "bmm": bench_bmm,
       "softmax": bench_softmax, "ln": bench_ln,
       "gn": bench_gn, "decode": bench_decode, "skinny": bench_skinny,
       "sample": bench_sample, "gradnorm": bench_gradnorm}

if __name__ == "__main__":
    which = sys.argv[1:] or list(ALL)
    for name in which:
        ALL[name]()
