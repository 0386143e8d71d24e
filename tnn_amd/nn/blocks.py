"""Blocks: layer compositions (reference include/nn/blocks_impl/).

``Sequential`` is the unit of pipeline-stage deployment, exactly as in the
reference (include/nn/blocks_impl/sequential.hpp:21): the partitioner slices
a Sequential into per-rank stage Sequentials, which round-trip through config.
"""

from __future__ import annotations

import math
from typing import List, Optional

import torch
import torch.nn as nn

from .. import ops
from .layer import Layer, register_layer, layer_from_config


@register_layer("sequential")
class Sequential(Layer):
    def __init__(self, layers: Optional[List[Layer]] = None, name: str = "sequential",
                 dtype: torch.dtype = torch.float32):
        super().__init__(name, dtype)
        self.layers = nn.ModuleList(layers or [])

    def forward(self, x, start: int = 0):
        from .layers import BatchNorm, Conv2D, Dropout
        n = len(self.layers)
        i = start
        while i < n:
            layer = self.layers[i]
            fuse = self.training and x.is_cuda
            # peephole: Conv2D -> BatchNorm(train) computes the BN batch
            # statistics in the conv epilogue (saves the stats pass's full
            # read of y); a following Dropout merges into the BN apply too
            if (fuse and isinstance(layer, Conv2D) and i + 1 < n
                    and isinstance(self.layers[i + 1], BatchNorm)):
                bn = self.layers[i + 1]
                drop = None
                if (i + 2 < n and bn.relu
                        and isinstance(self.layers[i + 2], Dropout)
                        and self.layers[i + 2].p > 0):
                    drop = self.layers[i + 2]
                y, stats = ops.conv2d_nhwc(x.to(layer.io_dtype), layer.weight,
                                           layer.bias, layer.stride,
                                           layer.padding, want_stats=True)
                x = ops.batch_norm_act(y, bn.gamma, bn.beta, bn.running_mean,
                                       bn.running_var, True, bn.momentum,
                                       bn.eps, bn.relu,
                                       drop.p if drop is not None else 0.0,
                                       precomputed=stats)
                i += 3 if drop is not None else 2
                continue
            # peephole: BN(relu) directly followed by Dropout runs as one
            # fused kernel pass on GPU during training (ops.batch_norm_act
            # dropout_p) -- saves the dropout read/write passes entirely
            if (fuse and i + 1 < n
                    and isinstance(layer, BatchNorm) and layer.relu
                    and isinstance(self.layers[i + 1], Dropout)
                    and self.layers[i + 1].p > 0):
                x = ops.batch_norm_act(x, layer.gamma, layer.beta,
                                       layer.running_mean, layer.running_var,
                                       True, layer.momentum, layer.eps,
                                       True, self.layers[i + 1].p)
                i += 2
                continue
            x = layer(x)
            i += 1
        return x

    def output_shape(self, in_shape):
        for layer in self.layers:
            in_shape = layer.output_shape(in_shape)
        return tuple(in_shape)

    def flops_per_item(self, in_shape):
        total = 0
        for layer in self.layers:
            total += layer.flops_per_item(in_shape)
            in_shape = layer.output_shape(in_shape)
        return total

    def slice(self, start: int, end: int, name: Optional[str] = None) -> "Sequential":
        """Sub-Sequential over layers [start, end) — used by the partitioner."""
        return Sequential(list(self.layers[start:end]),
                          name=name or f"{self.name}[{start}:{end}]")

    def __len__(self):
        return len(self.layers)

    def __iter__(self):
        return iter(self.layers)

    def extra_config(self):
        return {"layers": [l.get_config() for l in self.layers]}

    @classmethod
    def from_config(cls, cfg):
        cfg = dict(cfg)
        cfg.pop("type", None)
        cfg.pop("dtype", None)
        layers = [layer_from_config(c) for c in cfg.pop("layers", [])]
        return cls(layers, **cfg)


@register_layer("residual_block")
class ResidualBlock(Layer):
    """main + optional shortcut, add-join, final activation
    (reference src/nn/blocks_impl/residual_block.cpp:22-80)."""

    def __init__(self, main: Layer, shortcut: Optional[Layer] = None,
                 final_activation: str = "relu", name: str = "residual_block",
                 dtype: torch.dtype = torch.float32):
        super().__init__(name, dtype)
        self.main = main
        self.shortcut = shortcut
        self.final_activation = final_activation

    def forward(self, x):
        main = self.main
        from .layers import BatchNorm, Dropout
        if (x.is_cuda and self.training and isinstance(main, Sequential)
                and len(main.layers) > 0
                and isinstance(main.layers[0], BatchNorm)
                and not (len(main.layers) > 1
                         and isinstance(main.layers[1], Dropout))):
            # pre-activation block: the shortcut rides the first BN's
            # residual passthrough, so x keeps ONE consumer and the
            # junction grad join runs inside bn_bwd (no autograd add)
            y0, xr = main.layers[0].forward_res(x)
            y = main(y0, start=1)
            s = self.shortcut(xr) if self.shortcut is not None else xr
            return ops.add_act(y, s, self.final_activation)
        y = main(x)
        s = self.shortcut(x) if self.shortcut is not None else x
        return ops.add_act(y, s, self.final_activation)

    def output_shape(self, in_shape):
        return self.main.output_shape(in_shape)

    def flops_per_item(self, in_shape):
        f = self.main.flops_per_item(in_shape)
        if self.shortcut is not None:
            f += self.shortcut.flops_per_item(in_shape)
        return f + math.prod(self.main.output_shape(in_shape))

    def extra_config(self):
        return {"main": self.main.get_config(),
                "shortcut": self.shortcut.get_config() if self.shortcut else None,
                "final_activation": self.final_activation}

    @classmethod
    def from_config(cls, cfg):
        cfg = dict(cfg)
        cfg.pop("type", None)
        cfg.pop("dtype", None)
        main = layer_from_config(cfg.pop("main"))
        sc = cfg.pop("shortcut", None)
        shortcut = layer_from_config(sc) if sc else None
        return cls(main, shortcut, **cfg)


@register_layer("msequential")
class MSequential(Layer):
    """Parallel branches + elementwise join (reference msequential.cpp:40-89).

    Memory-aware branch scheduling (reference measure_sequence_memory /
    compute_execution_order): each branch is trial-run once on its first
    GPU forward while the caching allocator's peak/retained deltas are
    recorded; branches then execute sorted by priority = peak-workspace −
    retained bytes (descending), so high-transient / low-retained
    branches run while free memory is largest. The join always combines
    outputs in DECLARATION order (sub/div are not commutative), only the
    execution order changes.
    """

    JOINS = {"add": torch.add, "sub": torch.sub, "mul": torch.mul,
             "div": torch.div}

    def __init__(self, branches: List[Layer], join: str = "add",
                 name: str = "msequential", dtype: torch.dtype = torch.float32):
        super().__init__(name, dtype)
        self.branches = nn.ModuleList(branches)
        self.join = join
        self._exec_order: Optional[List[int]] = None

    def _measure_order(self, x) -> List[int]:
        """Reference SequenceMemInfo: one no-grad trial per branch,
        priority = cycling_cost − output_size, stable sort descending."""
        infos = []
        dev = x.device
        for i, b in enumerate(self.branches):
            torch.cuda.synchronize(dev)
            torch.cuda.reset_peak_memory_stats(dev)
            before = torch.cuda.memory_allocated(dev)
            with torch.no_grad():
                out = b(x)
            torch.cuda.synchronize(dev)
            peak = torch.cuda.max_memory_allocated(dev) - before
            retained = out.numel() * out.element_size()
            del out
            infos.append((peak - retained, i))
        infos.sort(key=lambda t: (-t[0], t[1]))
        return [i for _, i in infos]

    def forward(self, x):
        if self._exec_order is None:
            self._exec_order = (self._measure_order(x) if x.is_cuda
                                else list(range(len(self.branches))))
        outs: List[Optional[torch.Tensor]] = [None] * len(self.branches)
        for i in self._exec_order:
            outs[i] = self.branches[i](x)
        if self.join == "concat":
            return torch.cat(outs, dim=-1)
        if self.join == "add":
            y = outs[0]
            for o in outs[1:]:
                y = ops.add_act(y, o)
            return y
        fn = self.JOINS[self.join]
        y = outs[0]
        for o in outs[1:]:
            y = fn(y, o)
        return y

    def output_shape(self, in_shape):
        shapes = [b.output_shape(in_shape) for b in self.branches]
        if self.join == "concat":
            last = sum(s[-1] for s in shapes)
            return (*shapes[0][:-1], last)
        return shapes[0]

    def flops_per_item(self, in_shape):
        return sum(b.flops_per_item(in_shape) for b in self.branches)

    def extra_config(self):
        return {"branches": [b.get_config() for b in self.branches], "join": self.join}

    @classmethod
    def from_config(cls, cfg):
        cfg = dict(cfg)
        cfg.pop("type", None)
        cfg.pop("dtype", None)
        branches = [layer_from_config(c) for c in cfg.pop("branches")]
        return cls(branches, **cfg)


class _MHABase(Layer):
    """Shared q/k/v/o projection plumbing for attention blocks
    (reference src/nn/blocks_impl/attention_block.cpp:144)."""

    def __init__(self, dim: int, num_heads: int, causal: bool = True,
                 name: str = "attention", dtype: torch.dtype = torch.float32):
        super().__init__(name, dtype)
        assert dim % num_heads == 0
        self.dim, self.num_heads, self.causal = dim, num_heads, causal
        self.head_dim = dim // num_heads
        std = 0.02
        self.wq = nn.Parameter(torch.randn(dim, dim, dtype=dtype) * std)
        self.wk = nn.Parameter(torch.randn(dim, dim, dtype=dtype) * std)
        self.wv = nn.Parameter(torch.randn(dim, dim, dtype=dtype) * std)
        self.wo = nn.Parameter(torch.randn(dim, dim, dtype=dtype) * std)
        self.bq = nn.Parameter(torch.zeros(dim, dtype=dtype))
        self.bk = nn.Parameter(torch.zeros(dim, dtype=dtype))
        self.bv = nn.Parameter(torch.zeros(dim, dtype=dtype))
        self.bo = nn.Parameter(torch.zeros(dim, dtype=dtype))

    _kv_cache = None  # dict cache state; None = training mode
    _wqkv = None      # concatenated projection weights (decode fast path)

    def reset_cache(self):
        self._kv_cache = None
        self._wqkv = self._bqkv = None

    def _build_qkv_merge(self):
        """One [D, 3D] GEMV instead of three per decode step (the per-
        kernel floor dominates batch-1 decode; built once per cache
        session, dropped on reset)."""
        with torch.no_grad():
            self._wqkv = torch.cat([self.wq, self.wk, self.wv], 1).contiguous()
            self._bqkv = torch.cat([self.bq, self.bk, self.bv]).contiguous()

    def enable_cache(self, max_len: int = 1024):
        # buffers allocated lazily at prefill (batch size unknown here);
        # appends are in-place slice writes, never torch.cat reallocation
        self._kv_cache = {"k": None, "v": None, "len": 0, "cap": max_len}

    def enable_static_cache(self, max_len: int, pos_t: torch.Tensor):
        """hipGraph-capturable decode cache: every tensor shape is fixed at
        ``max_len`` and the current position lives in the shared int64
        device tensor ``pos_t`` ([1]), so a captured single-token step can
        be replayed with no host round-trips. Prefill (s>1) still runs the
        eager path; single-token steps write k/v at pos_t via index_copy_
        and attend over the full capacity with a pos_t-derived mask.
        ``pos_t`` may also be ``[B]``, one position per sequence of a
        ragged batch: the step then appends with ``ops.kv_append`` and
        every sequence attends over its own length."""
        self._kv_cache = {"k": None, "v": None, "len": 0, "cap": max_len,
                          "pos_t": pos_t}

    def set_extend(self, on: bool, n_new: Optional[torch.Tensor] = None,
                   kv_splits: int = 0):
        """Extend mode of the per-sequence static cache: a forward over
        ``[B, T]`` appends row b's first ``n_new[b]`` tokens (all T when
        None) at ``pos_t[b]`` and attends each over its own prefix
        (``_extend_forward``). Off, multi-token input keeps the prefill
        route, which writes at one shared host position. ``kv_splits``
        goes to ``ops.attention_extend`` (0: the unsplit kernel)."""
        c = self._kv_cache
        assert c is not None and "pos_t" in c and c["pos_t"].numel() >= 1
        c["extend"], c["n_new"] = on, n_new if on else None
        c["kv_splits"] = kv_splits if on else 0

    def _extending(self) -> bool:
        c = self._kv_cache
        return c is not None and bool(c.get("extend"))

    def _extend_forward(self, x, residual=None, ln=None):
        """One merged-QKV projection, one multi-row cache append, extend
        attention over each sequence's own prefix, view-only merge."""
        c = self._kv_cache
        b, s, d = x.shape
        h, hd = self.num_heads, self.head_dim
        if self._wqkv is None:
            self._build_qkv_merge()
        if s == 1 and x.is_cuda and not x.requires_grad:
            qkv = ops.linear(x, self._wqkv, self._bqkv, ln=ln)
        else:
            if ln is not None:
                x = ops.layer_norm(x, *ln)
            qkv = ops.linear(x, self._wqkv, self._bqkv)
        q, k, v = (t.view(b, s, h, hd).transpose(1, 2)
                   for t in qkv.detach().split(d, dim=-1))
        if c["k"] is None:
            c["k"] = torch.zeros(b, h, c["cap"], hd, device=x.device,
                                 dtype=k.dtype)
            c["v"] = torch.zeros_like(c["k"])
        ops.kv_append_n(c["k"], c["v"], k, v, c["pos_t"], c["n_new"])
        o = ops.attention_extend(q, c["k"], c["v"], c["pos_t"], c["n_new"],
                                 hd ** -0.5, c.get("kv_splits", 0))
        o = o.transpose(1, 2).reshape(b, s, d)   # [B,T,H,D] memory: a view
        return ops.linear(o, self.wo, self.bo, residual=residual)

    def _project(self, x, ln=None):
        b, s, d = x.shape
        h, hd = self.num_heads, self.head_dim
        if (self._kv_cache is not None and s == 1 and x.is_cuda
                and not x.requires_grad):
            if self._wqkv is None:
                self._build_qkv_merge()
            qkv = ops.linear(x, self._wqkv, self._bqkv, ln=ln)
            q, k, v = (t.view(b, s, h, hd).transpose(1, 2)
                       for t in qkv.split(d, dim=-1))
        else:
            if ln is not None:
                x = ops.layer_norm(x, *ln)
            q = ops.linear(x, self.wq, self.bq).view(b, s, h, hd).transpose(1, 2)
            k = ops.linear(x, self.wk, self.bk).view(b, s, h, hd).transpose(1, 2)
            v = ops.linear(x, self.wv, self.bv).view(b, s, h, hd).transpose(1, 2)
        c = self._kv_cache
        if c is not None:
            if c["k"] is None:
                c["k"] = torch.zeros(b, h, c["cap"], hd, device=x.device,
                                     dtype=k.dtype)
                c["v"] = torch.zeros_like(c["k"])
            if "pos_t" in c and s == 1:
                # graph-capturable single-token append at pos_t
                if c["pos_t"].numel() > 1:   # one position per sequence
                    ops.kv_append(c["k"], c["v"], k.detach(), v.detach(),
                                  c["pos_t"])
                    return q, c["k"], c["v"]
                c["k"].index_copy_(2, c["pos_t"], k.detach())
                c["v"].index_copy_(2, c["pos_t"], v.detach())
                return q, c["k"], c["v"]
            t0, t1 = c["len"], c["len"] + s
            c["k"][:, :, t0:t1] = k.detach()
            c["v"][:, :, t0:t1] = v.detach()
            c["len"] = t1
            k = c["k"][:, :, :t1]
            v = c["v"][:, :, :t1]
        return q, k, v

    def _cached_attention(self, q, k, v):
        """Decode-path attention: q covers the s_new newest positions of
        the k/v sequence; causal within the suffix, full over the prefix
        (the KV-cache fast path the reference lacks —
        examples/gpt2_inference.cpp recomputes the full sequence).

        GPU single-token steps run the fused decode-attention kernel
        (csrc/decode.hip — one split-KV pass + combine, replacing the
        matmul → mask → softmax → matmul chain); multi-token prefill runs
        batched MFMA GEMMs + the fused causal-softmax kernel. The static
        (pos_t) cache reads its live length from the device position
        tensor inside the kernel, so every shape stays fixed for hipGraph
        capture."""
        c = self._kv_cache
        t, s_new = k.shape[-2], q.shape[-2]
        scale = self.head_dim ** -0.5
        if (q.is_cuda and q.dtype == torch.bfloat16 and s_new == 1
                and c is not None and self.head_dim in (64, 128)
                and not q.requires_grad):
            b, h, _, hd = q.shape
            kc, vc = c["k"], c["v"]  # full [B,H,cap,D] buffers
            cap = kc.shape[2]
            o = ops.attention_decode(
                q.reshape(b * h, hd), kc.view(b * h, cap, hd),
                vc.view(b * h, cap, hd), c.get("pos_t"), t, scale)
            return o.view(b, h, 1, hd)
        if q.is_cuda and not (c is not None and "pos_t" in c and s_new == 1):
            # prefill / multi-token suffix: causal within the suffix with
            # offset t - s_new, full attention over the cached prefix
            return ops.sdpa_materialized(q, k, v, causal=self.causal,
                                         qoff=t - s_new)
        scores = torch.matmul(q.float(), k.float().transpose(-1, -2)) * scale
        if c is not None and "pos_t" in c and s_new == 1:
            if "arange" not in c:
                c["arange"] = torch.arange(c["cap"], device=q.device)
            if c["pos_t"].numel() > 1:   # [B, cap] -> over heads and the row
                dead = (c["arange"][None, :]
                        > c["pos_t"][:, None])[:, None, None, :]
            else:
                dead = c["arange"] > c["pos_t"]
            scores = scores.masked_fill(dead, float("-inf"))
        elif self.causal and s_new > 1:
            pos_q = torch.arange(t - s_new, t, device=q.device).unsqueeze(-1)
            pos_k = torch.arange(t, device=q.device)
            scores = scores.masked_fill(pos_k > pos_q, float("-inf"))
        p = torch.softmax(scores, dim=-1).to(v.dtype)
        return torch.matmul(p, v)

    def _merge(self, o, b, s, residual=None):
        o = o.transpose(1, 2).reshape(b, s, self.dim)
        # the transformer-block residual add rides the o-projection GEMM
        # epilogue when supplied (one fused kernel, no at::native add pass)
        return ops.linear(o, self.wo, self.bo, residual=residual)

    def output_shape(self, in_shape):
        return tuple(in_shape)

    def flops_per_item(self, in_shape):
        s, d = in_shape
        return 8 * s * d * d + 4 * s * s * d

    def extra_config(self):
        return {"dim": self.dim, "num_heads": self.num_heads, "causal": self.causal}


@register_layer("attention_block")
class AttentionBlock(_MHABase):
    """Materialized-scores attention (reference AttentionBlock): batched
    MFMA GEMMs + one fused scale/causal-mask softmax pass — no rocBLAS,
    no separate mask fill (reference attention_block.cpp:144-147,
    permute_heads.cu, causal_mask.cu, softmax.cu)."""

    def forward(self, x, residual=None, ln=None):
        b, s, _ = x.shape
        if self._extending():
            return self._extend_forward(x, residual, ln)
        q, k, v = self._project(x, ln=ln)
        if self._kv_cache is not None:
            o = self._cached_attention(q, k, v)
            return self._merge(o, b, s, residual)
        o = ops.sdpa_materialized(q, k, v, causal=self.causal)
        return self._merge(o, b, s, residual)


@register_layer("flash_attention_block")
class FlashAttentionBlock(_MHABase):
    """Flash attention via the hand-written CDNA4 kernel on GPU
    (reference FlashAttentionBlock / cudnn SDPA graph)."""

    def forward(self, x, residual=None, ln=None):
        b, s, _ = x.shape
        if self._extending():
            return self._extend_forward(x, residual, ln)
        if self._kv_cache is not None:
            q, k, v = self._project(x, ln=ln)
            o = self._cached_attention(q, k, v)
            return self._merge(o, b, s, residual)
        if (x.is_cuda and x.dtype == torch.bfloat16
                and self.head_dim in (64, 128)):
            # merged-QKV training path: one projection GEMM, attention
            # reads the head slices as strided views, dqkv comes back in
            # one buffer (no fan-in adds, no slice backwards)
            if ln is not None:
                x = ops.layer_norm(x, *ln)
            qkv = ops.linear_qkv(x, self.wq, self.wk, self.wv,
                                 self.bq, self.bk, self.bv)
            o = ops.flash_attention_qkv(qkv, self.num_heads, self.causal)
            return ops.linear(o, self.wo, self.bo, residual=residual)
        q, k, v = self._project(x, ln=ln)
        o = ops.attention(q, k, v, causal=self.causal)
        return self._merge(o, b, s, residual)


@register_layer("gpt_block")
class GPTBlock(Layer):
    """Pre-LN transformer block: ln→attn→res, ln→mlp(gelu)→res
    (reference gpt models, src/nn/example_models.cpp:384)."""

    def __init__(self, dim: int, num_heads: int, mlp_ratio: int = 4,
                 flash: bool = True, dropout: float = 0.0,
                 name: str = "gpt_block", dtype: torch.dtype = torch.float32):
        super().__init__(name, dtype)
        self.dim, self.num_heads = dim, num_heads
        self.mlp_ratio, self.flash, self.dropout_p = mlp_ratio, flash, dropout
        from .layers import LayerNorm, Dropout
        cls = FlashAttentionBlock if flash else AttentionBlock
        self.ln1 = LayerNorm(dim, name=f"{name}_ln1", dtype=dtype)
        self.attn = cls(dim, num_heads, causal=True, name=f"{name}_attn", dtype=dtype)
        self.ln2 = LayerNorm(dim, name=f"{name}_ln2", dtype=dtype)
        hidden = dim * mlp_ratio
        std = 0.02
        self.w1 = nn.Parameter(torch.randn(dim, hidden, dtype=dtype) * std)
        self.b1 = nn.Parameter(torch.zeros(hidden, dtype=dtype))
        self.w2 = nn.Parameter(torch.randn(hidden, dim, dtype=dtype) * std)
        self.b2 = nn.Parameter(torch.zeros(dim, dtype=dtype))
        self.drop = Dropout(dropout, name=f"{name}_drop", dtype=dtype) if dropout > 0 else None

    def forward(self, x):
        if (x.is_cuda and x.shape[1] == 1 and not torch.is_grad_enabled()
                and self.attn._kv_cache is not None):
            # decode fast path: both LayerNorms ride the projection GEMVs
            x = self.attn(x, residual=x,
                          ln=(self.ln1.gamma, self.ln1.beta, self.ln1.eps))
            h = ops.linear(x, self.w1, self.b1, act="gelu",
                           ln=(self.ln2.gamma, self.ln2.beta, self.ln2.eps))
            return ops.linear(h, self.w2, self.b2, residual=x)
        if x.is_cuda:
            # residual branches ride the LayerNorm passthrough outputs:
            # x/a keep ONE consumer each, so the junction grad joins run
            # inside ln_bwd (autograd fan-in adds removed — 2 activation
            # adds per block per step)
            ln1_out, xr = ops.layer_norm_res(x, self.ln1.gamma,
                                             self.ln1.beta, self.ln1.eps)
            a = self.attn(ln1_out, residual=xr)
            ln2_out, ar = ops.layer_norm_res(a, self.ln2.gamma,
                                             self.ln2.beta, self.ln2.eps)
            h = ops.linear(ln2_out, self.w1, self.b1, act="gelu")
            if self.drop is not None:
                h = self.drop(ops.linear(h, self.w2, self.b2))
                return ops.add_act(ar, h)
            return ops.linear(h, self.w2, self.b2, residual=ar)
        x = self.attn(self.ln1(x), residual=x)
        h = ops.linear(self.ln2(x), self.w1, self.b1, act="gelu")
        if self.drop is not None:
            h = self.drop(ops.linear(h, self.w2, self.b2))
            return x + h
        return ops.linear(h, self.w2, self.b2, residual=x)


    def flops_per_item(self, in_shape):
        s, d = in_shape
        return self.attn.flops_per_item(in_shape) + 4 * s * d * d * self.mlp_ratio

    def extra_config(self):
        return {"dim": self.dim, "num_heads": self.num_heads,
                "mlp_ratio": self.mlp_ratio, "flash": self.flash,
                "dropout": self.dropout_p}
