"""Functional ops with CPU(torch-composition) / GPU(HIP kernel) dispatch.

GPU autograd Functions call into the in-tree HIP extension; CPU paths are
pure differentiable torch compositions used as the numerics oracle
(reference unit_tests/layer_device_agnosticity_test.cpp:25 pattern).

All image ops are NHWC: x is a contiguous ``[N, H, W, C]`` tensor and conv
weights are ``[KH, KW, Cin, Cout]`` (the implicit-GEMM B-operand layout).
"""

from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.nn.functional as F

from .. import _C

# ---------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------

ACT_KINDS = {
    "linear": 0,
    "relu": 1,
    "gelu": 2,       # tanh approximation (reference gelu_kernels.cu:18)
    "sigmoid": 3,
    "tanh": 4,
    "elu": 5,
    "leaky_relu": 6,
    "silu": 7,
}


def _nhwc_to_nchw(x: torch.Tensor) -> torch.Tensor:
    return x.permute(0, 3, 1, 2)


def _nchw_to_nhwc(x: torch.Tensor) -> torch.Tensor:
    return x.permute(0, 2, 3, 1).contiguous()


def _use_hip(*tensors: torch.Tensor) -> bool:
    return any(t is not None and t.is_cuda for t in tensors)


# hipGraph-captured training steps: RNG consumers combine a per-call salt
# (baked at capture) with this device counter (incremented in-graph), so
# every replay draws a fresh Philox stream with zero host involvement.
_graph_ctr: Optional[torch.Tensor] = None


def set_graph_seed_ctr(t: Optional[torch.Tensor]):
    global _graph_ctr
    _graph_ctr = t


# Gradient sinks: a training step that owns fixed gradient buffers (the
# per-dtype slabs of GraphedTrainStep) registers them here, and the conv and
# batch-norm backwards then have their reduce kernels write dw / db / dgamma /
# dbeta straight into the buffer and hand autograd None for that input --
# instead of returning a fresh tensor that autograd adds to the zeroed buffer
# with one more launch per parameter. With no registry active (eager training,
# the pipeline engine, DDP) nothing changes.
class GradSinks:
    """Parameter -> gradient buffer, plus the per-step "written" marks.

    The first write of a step overwrites the buffer, any later write in the
    same step accumulates (a layer applied twice); ``begin_step`` clears the
    marks. Keys are the parameters' ``data_ptr()``: a backward sees the tensor
    that reached its forward, which is the parameter or an alias of it."""

    def __init__(self, params=()):
        self._buf = {}
        self.written = set()
        for p in params:
            self.register(p, p.grad)

    def register(self, param: torch.Tensor, buf: torch.Tensor):
        if (buf is None or buf.shape != param.shape or buf.dtype != param.dtype
                or buf.device != param.device or not buf.is_contiguous()):
            raise ValueError("gradient sink must be a contiguous buffer of the "
                             "parameter's shape, dtype and device")
        self._buf[param.data_ptr()] = buf

    def begin_step(self):
        self.written.clear()

    def get(self, key, like: Optional[torch.Tensor] = None):
        """The buffer registered under ``key`` (None if there is none, or if
        it does not match the shape and dtype of ``like``)."""
        buf = self._buf.get(key)
        if buf is not None and like is not None and (
                buf.shape != like.shape or buf.dtype != like.dtype):
            return None
        return buf

    def claim(self, key) -> bool:
        """Mark ``key`` written in this step; returns whether the write has
        to accumulate (it was written before in the same step)."""
        accumulate = key in self.written
        self.written.add(key)
        return accumulate


_grad_sinks: Optional[GradSinks] = None


def grad_sinks_enabled() -> bool:
    """``TNN_GRAD_SINK=0`` turns the gradient sinks off."""
    import os
    return os.environ.get("TNN_GRAD_SINK", "1") != "0"


def set_grad_sinks(sinks: Optional[GradSinks]):
    global _grad_sinks
    _grad_sinks = sinks


def _sink_key(t: Optional[torch.Tensor]):
    # recorded in forward, from the tensor as the layer passed it. Only a
    # contiguous tensor can be the parameter itself: a same-shape view with
    # other strides (a transposed square weight) shares the pointer but not
    # the element order, and gets its gradient from autograd
    if (_grad_sinks is None or t is None or not t.requires_grad
            or not t.is_contiguous()):
        return None
    return t.data_ptr()


def _draw_seed() -> int:
    if _graph_ctr is not None:
        import random
        return random.getrandbits(62)  # salt only; no GPU sync in capture
    return int(torch.randint(0, 2 ** 62, (1,)).item())


# ---------------------------------------------------------------------------
# conv2d NHWC (implicit GEMM on GPU; reference legacy_conv2d_layer.cpp:137)
# ---------------------------------------------------------------------------


class _Conv2dNHWC(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, bias, stride, padding, fuse_relu, want_stats=False):
        ext = _C.ext()
        # narrow-channel inputs (the RGB stem) fall off every vector/glds
        # path (measured 192us vs ~35 for the padded form): zero-pad Cin to
        # the 16B vector width once -- zero channels contribute nothing
        Ci = x.shape[-1]
        V = 8 if x.dtype == torch.bfloat16 else 4
        ctx.cin = Ci
        ctx.sink_keys = (_sink_key(w), _sink_key(bias))
        if Ci % V != 0 and Ci < V:
            x = F.pad(x, (0, V - Ci))
            w = F.pad(w, (0, 0, 0, V - Ci))
        ctx.want_stats = want_stats
        if want_stats:
            # fused per-channel sum/sumsq for a following train-mode BN, as
            # slab partials [m-tiles, 2, Cout] that bn_fwd_train folds in its
            # finalize; empty when the fused kernel is not eligible
            y, stats = ext.conv2d_fwd_partials(x, w, bias, stride[0],
                                               stride[1], padding[0],
                                               padding[1])
        else:
            y = ext.conv2d_fwd(x, w, bias, stride[0], stride[1], padding[0],
                               padding[1], fuse_relu)
        ctx.save_for_backward(x, w, y if fuse_relu else None)
        ctx.stride, ctx.padding, ctx.fuse_relu = stride, padding, fuse_relu
        ctx.has_bias = bias is not None
        if want_stats:
            # non-differentiable alone does not keep autograd from filling a
            # zero [2, Cout] gradient for stats on every backward (one fill
            # per fused-statistics conv and step, seen in the profiler)
            ctx.mark_non_differentiable(stats)
            ctx.set_materialize_grads(False)
            return y, stats
        return y

    @staticmethod
    def backward(ctx, dy, *unused_stats_grad):
        if dy is None:  # y unused (grads are not materialized with stats)
            return None, None, None, None, None, None, None
        x, w, y = ctx.saved_tensors
        ext = _C.ext()
        dy = dy.contiguous()
        if ctx.fuse_relu:
            dy = ext.relu_bwd_mask(dy, y)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = ext.conv2d_dgrad(dy, w, x.shape[1], x.shape[2],
                                  ctx.stride[0], ctx.stride[1], ctx.padding[0], ctx.padding[1])
            if x.shape[-1] != ctx.cin:
                dx = dx[..., :ctx.cin].contiguous()
        want_db = ctx.has_bias and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1] and _grad_sinks is not None:
            sunk = _Conv2dNHWC._wgrad_into_sinks(ctx, x, w, dy, want_db)
            if sunk is not None:
                return (dx,) + sunk + (None, None, None, None)
        if ctx.needs_input_grad[1]:
            args = (x, dy, w.shape[0], w.shape[1], ctx.stride[0],
                    ctx.stride[1], ctx.padding[0], ctx.padding[1],
                    w.dtype == x.dtype)
            if want_db:
                # the bias gradient rides along as one more wgrad output
                # row: no second pass over dy, no separate cast
                dw, db = ext.conv2d_wgrad_bias(*args)
                db = db.to(dy.dtype)  # no-op when the reduce already cast
            else:
                dw = ext.conv2d_wgrad(*args)
            if x.shape[-1] != ctx.cin:
                dw = dw[:, :, :ctx.cin].contiguous()
            dw = dw.to(w.dtype)  # no-op when the reduce already cast
        elif want_db:
            db = ext.colsum(dy.reshape(-1, dy.shape[-1]))
        return dx, dw, db, None, None, None, None

    @staticmethod
    def _wgrad_into_sinks(ctx, x, w, dy, want_db):
        """Weight (and bias) gradient through the registered sinks: returns
        the (dw, db) to hand autograd -- None where the reduce wrote the
        buffer -- or None when this layer goes the old way. The padded RGB
        stem keeps dw on the old path (it is sliced out of the padded
        gradient) but still sinks db."""
        sinks = _grad_sinks
        wkey, bkey = ctx.sink_keys
        padded = x.shape[-1] != ctx.cin
        dwbuf = dbbuf = None
        if w.dtype not in (x.dtype, torch.float32):
            return None
        if not padded:
            dwbuf = sinks.get(wkey, w)
            if dwbuf is None:
                return None
        if want_db:
            dbbuf = sinks.get(bkey, w[0, 0, 0])
            if dbbuf is None:
                return None
        if dwbuf is None and dbbuf is None:
            return None
        if (dwbuf is not None and dbbuf is not None
                and (wkey in sinks.written) != (bkey in sinks.written)):
            return None  # one reduce, one accumulate flag
        ext = _C.ext()
        acc = False
        if dwbuf is not None:
            acc = sinks.claim(wkey)
        if dbbuf is not None:
            acc = sinks.claim(bkey)
        dw = None
        if padded:
            # accumulate into a scratch dw would read garbage: zero it then
            dwbuf = (torch.zeros if acc else torch.empty)(
                w.shape, dtype=w.dtype, device=w.device)
            dw = dwbuf
        ext.conv2d_wgrad_into(x, dy, w.shape[0], w.shape[1], ctx.stride[0],
                              ctx.stride[1], ctx.padding[0], ctx.padding[1],
                              dwbuf, dbbuf, acc)
        if padded:
            dw = dw[:, :, :ctx.cin].contiguous()
        return dw, None


def conv2d_nhwc(
    x: torch.Tensor,
    w: torch.Tensor,
    bias: Optional[torch.Tensor] = None,
    stride: Tuple[int, int] = (1, 1),
    padding: Tuple[int, int] = (0, 0),
    fuse_relu: bool = False,
    want_stats: bool = False,
):
    """2-D convolution, NHWC activations, ``[KH,KW,Cin,Cout]`` weights.

    ``want_stats=True`` (GPU, linear act) additionally returns the fused
    per-channel (sum, sumsq) for a following train-mode BatchNorm as slab
    partials ``[m-tiles, 2, Cout]`` (``batch_norm_act(precomputed=...)``
    takes them as they are), or None when the fused kernel is not
    eligible."""
    if _use_hip(x):
        if want_stats:
            y, stats = _Conv2dNHWC.apply(
                x.contiguous(), w.contiguous(),
                None if bias is None else bias.contiguous(), stride, padding,
                False, True)
            return y, (stats if stats.numel() else None)
        return _Conv2dNHWC.apply(x.contiguous(), w.contiguous(),
                                 None if bias is None else bias.contiguous(),
                                 stride, padding, fuse_relu)
    wn = w.permute(3, 2, 0, 1)  # -> [Cout, Cin, KH, KW]
    y = F.conv2d(_nhwc_to_nchw(x), wn, bias, stride=stride, padding=padding)
    if want_stats:
        return _nchw_to_nhwc(y), None
    y = _nchw_to_nhwc(y)
    if fuse_relu:
        y = F.relu(y)
    return y


# ---------------------------------------------------------------------------
# batch norm (+ fused ReLU) NHWC; stats always fp32
# (reference src/nn/layers_impl/batchnorm_layer.cpp:133-149)
# ---------------------------------------------------------------------------


def _bn_sinks(ctx, x, dy) -> dict:
    """bn_bwd keyword arguments that send dgamma / dbeta to the registered
    sinks; empty when the layer returns them the old way (no sink for both,
    one of them not wanted, or the scalar path, which has no finalize)."""
    sinks = _grad_sinks
    if sinks is None or not (ctx.needs_input_grad[1]
                             and ctx.needs_input_grad[2]):
        return {}
    gkey, bkey = ctx.sink_keys
    gbuf, bbuf = sinks.get(gkey), sinks.get(bkey)
    if (gbuf is None or bbuf is None or gbuf.dtype != torch.float32
            or bbuf.dtype != torch.float32
            or (gkey in sinks.written) != (bkey in sinks.written)
            or not _C.ext().bn_bwd_takes_sink(x, dy)):
        return {}
    sinks.claim(gkey)
    return dict(dgamma_out=gbuf, dbeta_out=bbuf, accumulate=sinks.claim(bkey))


class _BatchNormAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, momentum,
                eps, relu, dropout_p=0.0, seed=0, precomp=None, ctr=None):
        ext = _C.ext()
        # running stats update fused into the finalize kernel; dropout (if
        # any) fused into the apply kernel -- dropped positions write 0, so
        # the saved output doubles as relu mask and dropout mask and the
        # backward is a constant 1/(1-p) scale on the kept positions
        y, mean, invstd = ext.bn_fwd_train(x, gamma, beta, running_mean,
                                           running_var, momentum, eps, relu,
                                           dropout_p, seed, precomp, ctr)
        save_y = y if (relu or dropout_p > 0.0) else None
        ctx.save_for_backward(x, gamma, mean, invstd, save_y)
        ctx.sink_keys = (_sink_key(gamma), _sink_key(beta))
        ctx.relu = relu or dropout_p > 0.0
        ctx.dy_scale = 1.0 / (1.0 - dropout_p) if dropout_p > 0.0 else 1.0
        # mean/invstd carry no gradient; without set_materialize_grads(False)
        # autograd still fills a zero grad for each on every backward (2 fill
        # launches per BN per step, seen in the profiler)
        ctx.mark_non_differentiable(mean, invstd)
        ctx.set_materialize_grads(False)
        return y, mean, invstd

    @staticmethod
    def backward(ctx, dy, _dmean, _dinvstd):
        if dy is None:
            return (None,) * 12
        x, gamma, mean, invstd, y = ctx.saved_tensors
        ext = _C.ext()
        dy = dy.contiguous()
        sink = _bn_sinks(ctx, x, dy)
        dx, dgamma, dbeta = ext.bn_bwd(x, dy, gamma, mean, invstd,
                                       y if ctx.relu else None, ctx.dy_scale,
                                       **sink)
        if sink:
            dgamma = dbeta = None
        return (dx, dgamma, dbeta, None, None, None, None, None, None, None,
                None, None)


class _BatchNormActRes(torch.autograd.Function):
    """_BatchNormAct plus a residual PASSTHROUGH output (pre-activation
    residual blocks: the block input's junction grad join d_x = bn_grad +
    d_residual runs inside the bn_bwd apply kernel — no autograd fan-in
    add pass; mirrors _LayerNormRes)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, momentum,
                eps, relu, dropout_p, seed, precomp, ctr):
        ext = _C.ext()
        y, mean, invstd = ext.bn_fwd_train(x, gamma, beta, running_mean,
                                           running_var, momentum, eps, relu,
                                           dropout_p, seed, precomp, ctr)
        save_y = y if (relu or dropout_p > 0.0) else None
        ctx.save_for_backward(x, gamma, mean, invstd, save_y)
        ctx.sink_keys = (_sink_key(gamma), _sink_key(beta))
        ctx.relu = relu or dropout_p > 0.0
        ctx.dy_scale = 1.0 / (1.0 - dropout_p) if dropout_p > 0.0 else 1.0
        ctx.mark_non_differentiable(mean, invstd)
        ctx.set_materialize_grads(False)
        return y, mean, invstd, x.view_as(x)

    @staticmethod
    def backward(ctx, dy, _dm, _di, dres):
        x, gamma, mean, invstd, y = ctx.saved_tensors
        ext = _C.ext()
        if dy is None:
            return (dres, None, None, None, None, None, None, None, None,
                    None, None, None)
        if dres is not None:
            dres = dres.contiguous()
        dy = dy.contiguous()
        sink = _bn_sinks(ctx, x, dy)
        dx, dgamma, dbeta = ext.bn_bwd(x, dy, gamma, mean, invstd,
                                       y if ctx.relu else None, ctx.dy_scale,
                                       resid=dres, **sink)
        if sink:
            dgamma = dbeta = None
        return (dx, dgamma, dbeta, None, None, None, None, None, None, None,
                None, None)


def batch_norm_act(
    x: torch.Tensor,
    gamma: torch.Tensor,
    beta: torch.Tensor,
    running_mean: torch.Tensor,
    running_var: torch.Tensor,
    training: bool,
    momentum: float = 0.1,
    eps: float = 1e-5,
    relu: bool = False,
    dropout_p: float = 0.0,
    precomputed: Optional[torch.Tensor] = None,
    passthrough: bool = False,
):
    """BatchNorm over NHWC channels-last with optional fused ReLU and
    (train-time) fused dropout.

    Returns y. Updates running stats in-place when training (fp32, unbiased
    variance, matching torch semantics). gamma/beta/running stats are fp32
    regardless of x dtype (reference batchnorm_layer.cpp:140-148).
    dropout_p > 0 (requires relu) folds the dropout mask + 1/(1-p) scale
    into the BN apply kernel -- one memory pass instead of three.
    ``passthrough=True`` additionally returns x as a residual-branch
    alias whose grad joins inside bn_bwd (see _BatchNormActRes).
    """
    C = x.shape[-1]
    n = x.numel() // C
    if _use_hip(x):
        if training:
            seed = _draw_seed() if dropout_p > 0.0 else 0
            if passthrough:
                y, _, _, xr = _BatchNormActRes.apply(
                    x.contiguous(), gamma, beta, running_mean, running_var,
                    momentum, eps, relu, dropout_p, seed, precomputed,
                    _graph_ctr)
                return y, xr
            y, _, _ = _BatchNormAct.apply(x.contiguous(), gamma, beta,
                                          running_mean, running_var, momentum,
                                          eps, relu, dropout_p, seed,
                                          precomputed, _graph_ctr)
            return y
        ext = _C.ext()
        return ext.bn_fwd_infer(x.contiguous(), gamma, beta, running_mean, running_var,
                                eps, relu)
    # CPU reference path
    xf = x.reshape(-1, C).float()
    if training:
        mean = xf.mean(0)
        var = xf.var(0, unbiased=False)
        with torch.no_grad():
            running_mean.mul_(1 - momentum).add_(mean.detach(), alpha=momentum)
            running_var.mul_(1 - momentum).add_(var.detach() * (n / max(n - 1, 1)),
                                                alpha=momentum)
    else:
        mean, var = running_mean, running_var
    xhat = (x.float() - mean) / torch.sqrt(var + eps)
    y = xhat * gamma + beta
    if relu:
        y = F.relu(y)
    if dropout_p > 0.0 and training:
        y = F.dropout(y, dropout_p, training=True)
    y = y.to(x.dtype)
    return (y, x) if passthrough else y


# ---------------------------------------------------------------------------
# dense / GEMM (reference src/nn/layers_impl/cuda/dense_ops.cu:17-117)
# ---------------------------------------------------------------------------


class _Linear(torch.autograd.Function):
    """y = act(x @ w + b) [+ residual] — the residual add rides the GEMM
    epilogue (one fused kernel instead of a separate at::native
    elementwise pass; reference dense_ops.cu has no analog)."""

    @staticmethod
    def forward(ctx, x, w, bias, act, residual=None):
        ext = _C.ext()
        # every GEMM route computes act(xw + b) + residual, so forward may
        # fuse any pair; linear() refuses relu + residual with grad enabled
        # and backward refuses to replay a mask from such a y
        y = ext.gemm(x, w, bias, ACT_KINDS[act], residual)
        ctx.save_for_backward(x, w, y if act != "linear" else None)
        ctx.act = act
        ctx.has_bias = bias is not None
        ctx.has_res = residual is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        ext = _C.ext()
        dy = dy.contiguous()
        dres = dy if ctx.has_res else None
        if ctx.act == "relu":
            assert not ctx.has_res, \
                "fused residual requires act='linear' (relu mask would include it)"
            dy = ext.relu_bwd_mask(dy, y)
        elif ctx.act != "linear":
            raise NotImplementedError(f"fused act bwd for {ctx.act}")
        dx = dw = db = None
        N = dy.shape[-1]
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = ext.colsum(dy)
        # ragged N (e.g. the gpt2 vocab head, N=50257) forces every backward
        # GEMM onto the scalar-gather fallback (~75 TF vs ~450). Zero-pad dy
        # and w along N once: identical contraction, vector/glds kernels
        # throughout (measured 5.7x on the head's dgrad at seq 512).
        V = 8 if dy.dtype == torch.bfloat16 else 4
        pad = (-N) % V
        if pad and dy.shape[0] >= 64:
            dy_p = F.pad(dy, (0, pad))
            if ctx.needs_input_grad[0]:
                dx = ext.gemm_nt(dy_p, F.pad(w, (0, pad)))
            if ctx.needs_input_grad[1]:
                dw = ext.gemm_tn(x, dy_p, w.dtype == x.dtype)
                dw = dw[:, :N].contiguous().to(w.dtype)
            return dx, dw, db, None, dres
        if ctx.needs_input_grad[0]:
            dx = ext.gemm_nt(dy, w)       # [M,N] @ [K,N]^T -> [M,K]
        if ctx.needs_input_grad[1]:
            dw = ext.gemm_tn(x, dy, w.dtype == x.dtype)
            dw = dw.to(w.dtype)  # no-op when the reduce already cast
        return dx, dw, db, None, dres


class _LinearQKV(torch.autograd.Function):
    """The three attention projections as ONE GEMM: wqkv = cat(wq,wk,wv)
    rebuilt per call (a weight-sized copy, ~1% of the GEMM it replaces);
    3x fewer GEMM/colsum launches and the shared input x keeps a single
    consumer (no autograd fan-in adds). Weight/bias grads come back as
    contiguous slices of the single dW/db reductions."""

    @staticmethod
    def forward(ctx, x2, wq, wk, wv, bq, bk, bv):
        ext = _C.ext()
        wqkv = torch.cat([wq, wk, wv], dim=1)
        has_b = bq is not None
        bqkv = torch.cat([bq, bk, bv]) if has_b else None
        qkv = ext.gemm(x2, wqkv, bqkv, ACT_KINDS["linear"])
        ctx.save_for_backward(x2, wqkv)
        ctx.has_b = has_b
        return qkv

    @staticmethod
    def backward(ctx, dy):
        x2, wqkv = ctx.saved_tensors
        ext = _C.ext()
        dy = dy.contiguous()
        N = wqkv.shape[1] // 3
        dx = dwq = dwk = dwv = dbq = dbk = dbv = None
        if ctx.has_b and ctx.needs_input_grad[4]:
            db = ext.colsum(dy)
            dbq, dbk, dbv = db[:N], db[N:2 * N], db[2 * N:]
        if ctx.needs_input_grad[0]:
            dx = ext.gemm_nt(dy, wqkv)
        if ctx.needs_input_grad[1]:
            dw = ext.gemm_tn(x2, dy, wqkv.dtype == x2.dtype).to(wqkv.dtype)
            # contiguous slices: the fused multi-tensor optimizer reads
            # grads as flat buffers
            dwq = dw[:, :N].contiguous()
            dwk = dw[:, N:2 * N].contiguous()
            dwv = dw[:, 2 * N:].contiguous()
        return dx, dwq, dwk, dwv, dbq, dbk, dbv


def linear_qkv(x: torch.Tensor, wq, wk, wv, bq=None, bk=None, bv=None):
    """Merged attention projection: [.., K] -> [.., 3N] (see _LinearQKV)."""
    if not _use_hip(x):
        outs = [x @ w + (b if b is not None else 0)
                for w, b in ((wq, bq), (wk, bk), (wv, bv))]
        return torch.cat(outs, dim=-1)
    lead = x.shape[:-1]
    x2 = x.reshape(-1, x.shape[-1])
    y = _LinearQKV.apply(x2.contiguous(), wq, wk, wv, bq, bk, bv)
    return y.reshape(*lead, y.shape[-1])


def linear(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None,
           act: str = "linear",
           residual: Optional[torch.Tensor] = None,
           ln: Optional[tuple] = None) -> torch.Tensor:
    """y = act(ln?(x) @ w + bias) [+ residual]; x ``[..., K]``, w ``[K, N]``
    row-major. ``residual`` (shape of y) fuses the add into the GEMM
    epilogue on GPU (under no_grad together with any activation; with
    grad enabled act='relu' plus a residual is an error, other
    activations run unfused). ``ln=(gamma, beta, eps)``
    fuses a LayerNorm of x into the decode GEMV's staging (M=1,
    inference only). Under no_grad on GPU, 2 <= M <= 16 rows (batched
    decode) take the skinny GEMM, which reads every weight once for all
    rows and fuses ``ln`` too; ``TNN_SKINNY=0`` turns that route off."""
    lead = x.shape[:-1]
    x2 = x.reshape(-1, x.shape[-1])
    if (_use_hip(x) and 2 <= x2.shape[0] <= 16
            and not torch.is_grad_enabled()
            and x.dtype in (torch.float32, torch.bfloat16)
            and _C.ext().skinny_enabled()):
        gamma, beta, eps = ln if ln is not None else (None, None, 1e-5)
        y = _C.ext().gemm_skinny(
            x2.contiguous(), w.contiguous(),
            None if bias is None else bias.contiguous(), ACT_KINDS[act],
            residual.reshape(-1, residual.shape[-1]).contiguous()
            if residual is not None else None,
            gamma, beta, eps)
        return y.reshape(*lead, w.shape[1])
    if ln is not None:
        gamma, beta, eps = ln
        if (_use_hip(x) and x2.shape[0] == 1
                and not torch.is_grad_enabled()):
            ext = _C.ext()
            y = ext.gemm(x2.contiguous(), w, bias, ACT_KINDS[act],
                         residual.reshape(1, -1).contiguous()
                         if residual is not None else None,
                         gamma, beta, eps)
            return y.reshape(*lead, w.shape[1])
        x = layer_norm(x, gamma, beta, eps)
        x2 = x.reshape(-1, x.shape[-1])
    if _use_hip(x):
        # relu fuses into the GEMM epilogue (mask-replay backward); other
        # activations need the pre-activation saved, so run them unfused —
        # except under no_grad (decode), where any activation fuses
        fused = act if (act in ("linear", "relu")
                        or not torch.is_grad_enabled()) else "linear"
        r2 = (residual.reshape(-1, residual.shape[-1]).contiguous()
              if residual is not None else None)
        # with grad enabled a fused relu + residual stays an error: the
        # backward's mask replay reads y, which would include the residual
        assert (r2 is None or fused != "relu"
                or not torch.is_grad_enabled()), \
            "fused residual requires act='linear' when grad is enabled"
        y = _Linear.apply(x2.contiguous(), w.contiguous(),
                          None if bias is None else bias.contiguous(), fused,
                          r2 if fused == act else None)
        if fused != act:
            y = _Activation.apply(y, act)
            if residual is not None:
                y = y + r2
    else:
        y = x2 @ w
        if bias is not None:
            y = y + bias
        if act == "relu":
            y = F.relu(y)
        elif act == "gelu":
            y = F.gelu(y, approximate="tanh")
        elif act != "linear":
            y = activation(y, act)
        if residual is not None:
            y = y + residual.reshape(-1, residual.shape[-1])
    return y.reshape(*lead, w.shape[1])


class _Bmm(torch.autograd.Function):
    """Strided-batched MFMA GEMM (reference gemm_strided_batched_ex,
    src/math/cuda/gemm.cu:84-105). Transpose views pass through as
    strides — no materialized transposes anywhere in fwd or bwd."""

    @staticmethod
    def forward(ctx, a, b):
        ext = _C.ext()
        ctx.save_for_backward(a, b)
        return ext.bmm(a, b)

    @staticmethod
    def backward(ctx, dc):
        a, b = ctx.saved_tensors
        ext = _C.ext()
        da = db = None
        if ctx.needs_input_grad[0]:
            da = ext.bmm(dc, b.transpose(-1, -2))
        if ctx.needs_input_grad[1]:
            db = ext.bmm(a.transpose(-1, -2), dc)
        return da, db


def matmul(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Plain 2-D/batched matmul through the HIP MFMA GEMMs on GPU."""
    if _use_hip(a, b):
        if a.dim() == 2 and b.dim() == 2:
            return _Linear.apply(a.contiguous(), b.contiguous(), None, "linear")
        lead = a.shape[:-2]
        a3 = a.reshape(-1, a.shape[-2], a.shape[-1])
        b3 = b.reshape(-1, b.shape[-2], b.shape[-1])
        return _Bmm.apply(a3, b3).reshape(*lead, a.shape[-2], b.shape[-1])
    return a @ b


# ---------------------------------------------------------------------------
# pooling NHWC (reference maxpool_ops.cu / avgpool_ops.cu)
# ---------------------------------------------------------------------------


class _MaxPool2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, kernel, stride, padding):
        ext = _C.ext()
        y, idx = ext.maxpool_fwd(x, kernel[0], kernel[1], stride[0], stride[1],
                                 padding[0], padding[1])
        ctx.save_for_backward(idx)
        ctx.in_shape = x.shape
        return y

    @staticmethod
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        ext = _C.ext()
        dx = ext.maxpool_bwd(dy.contiguous(), idx, ctx.in_shape[1], ctx.in_shape[2])
        return dx, None, None, None


class _AvgPool2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, kernel, stride, padding):
        ext = _C.ext()
        y = ext.avgpool_fwd(x, kernel[0], kernel[1], stride[0], stride[1],
                            padding[0], padding[1])
        ctx.in_shape = x.shape
        ctx.kernel, ctx.stride, ctx.padding = kernel, stride, padding
        return y

    @staticmethod
    def backward(ctx, dy):
        ext = _C.ext()
        dx = ext.avgpool_bwd(dy.contiguous(), ctx.in_shape[1], ctx.in_shape[2],
                             ctx.kernel[0], ctx.kernel[1], ctx.stride[0], ctx.stride[1],
                             ctx.padding[0], ctx.padding[1])
        return dx, None, None, None


def max_pool2d_nhwc(x, kernel, stride=None, padding=(0, 0)):
    stride = stride or kernel
    if _use_hip(x):
        return _MaxPool2d.apply(x.contiguous(), kernel, stride, padding)
    y = F.max_pool2d(_nhwc_to_nchw(x), kernel, stride, padding)
    return _nchw_to_nhwc(y)


def avg_pool2d_nhwc(x, kernel, stride=None, padding=(0, 0)):
    stride = stride or kernel
    if _use_hip(x):
        return _AvgPool2d.apply(x.contiguous(), kernel, stride, padding)
    y = F.avg_pool2d(_nhwc_to_nchw(x), kernel, stride, padding)
    return _nchw_to_nhwc(y)


# ---------------------------------------------------------------------------
# dropout (Philox mask on GPU; reference dropout.cu:33)
# ---------------------------------------------------------------------------


class _Dropout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p, seed, ctr=None):
        ext = _C.ext()
        y, mask = ext.dropout_fwd(x, p, seed, ctr)
        ctx.save_for_backward(mask)
        ctx.p = p
        return y

    @staticmethod
    def backward(ctx, dy):
        (mask,) = ctx.saved_tensors
        ext = _C.ext()
        return (ext.dropout_bwd(dy.contiguous(), mask, ctx.p), None, None,
                None)


def dropout(x: torch.Tensor, p: float, training: bool) -> torch.Tensor:
    if not training or p <= 0.0:
        return x
    if _use_hip(x):
        return _Dropout.apply(x.contiguous(), p, _draw_seed(), _graph_ctr)
    return F.dropout(x, p, training=True)


# ---------------------------------------------------------------------------
# standalone activations (reference src/nn/activations_impl/)
# ---------------------------------------------------------------------------


class _Activation(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, kind):
        ext = _C.ext()
        y = ext.act_fwd(x, ACT_KINDS[kind])
        ctx.save_for_backward(x, y)
        ctx.kind = kind
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y = ctx.saved_tensors
        ext = _C.ext()
        return ext.act_bwd(dy.contiguous(), x, y, ACT_KINDS[ctx.kind]), None


class _ScaledSoftmax(torch.autograd.Function):
    """Row softmax with fused scale + causal mask (replaces the reference's
    causal_mask.cu fill + cudnnSoftmaxForward/Backward pair and the
    softmax activation kernels, softmax_kernels.cu:11-346)."""

    @staticmethod
    def forward(ctx, x, scale, causal, mrows, qoff):
        ext = _C.ext()
        y = ext.smax_fwd(x, mrows, qoff, scale, causal)
        ctx.save_for_backward(y)
        ctx.scale = scale
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        ext = _C.ext()
        dx = ext.smax_bwd(y, dy.contiguous(), ctx.scale)
        return dx, None, None, None, None


def scaled_softmax(x: torch.Tensor, scale: float = 1.0, causal: bool = False,
                   qoff: int = 0) -> torch.Tensor:
    """softmax(x * scale) over the last dim; with ``causal``, row r of each
    trailing [M, C] matrix may attend to columns <= r + qoff (suffix-causal
    decode prefill passes qoff = kv_len - M). Fully masked rows are 0."""
    if _use_hip(x):
        mrows = x.shape[-2] if x.dim() >= 2 else 1
        return _ScaledSoftmax.apply(x.contiguous(), scale, causal, mrows, qoff)
    xf = x.float() * scale
    if causal:
        M, C = x.shape[-2], x.shape[-1]
        pos_q = torch.arange(M, device=x.device).unsqueeze(-1) + qoff
        pos_k = torch.arange(C, device=x.device)
        xf = xf.masked_fill(pos_k > pos_q, float("-inf"))
    y = F.softmax(xf, dim=-1)
    y = torch.nan_to_num(y, nan=0.0)  # fully-masked rows -> 0 (kernel parity)
    return y.to(x.dtype)


class _AddAct(torch.autograd.Function):
    """y = act(a + b) in one pass (ResidualBlock join; backward is one
    shared mask pass for both inputs). Only y-derivable activations
    (relu/sigmoid/tanh/linear)."""

    @staticmethod
    def forward(ctx, a, b, kind):
        ext = _C.ext()
        y = ext.add_act_fwd(a, b, ACT_KINDS[kind])
        ctx.save_for_backward(y)
        ctx.kind = kind
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        ext = _C.ext()
        g = ext.add_act_bwd(dy.contiguous(), y, ACT_KINDS[ctx.kind])
        return g, g, None


def add_act(a: torch.Tensor, b: torch.Tensor,
            act: str = "linear") -> torch.Tensor:
    """Fused act(a + b) (residual joins)."""
    if act == "none":
        act = "linear"
    if (_use_hip(a, b) and a.shape == b.shape and a.dtype == b.dtype
            and act in ("linear", "relu", "sigmoid", "tanh")):
        return _AddAct.apply(a.contiguous(), b.contiguous(), act)
    y = a + b
    return activation(y, act) if act != "linear" else y


def activation(x: torch.Tensor, kind: str) -> torch.Tensor:
    if kind == "linear":
        return x
    if kind == "softmax":
        if _use_hip(x):
            return scaled_softmax(x, 1.0)
        return F.softmax(x, dim=-1)
    if _use_hip(x):
        return _Activation.apply(x.contiguous(), kind)
    if kind == "relu":
        return F.relu(x)
    if kind == "gelu":
        return F.gelu(x, approximate="tanh")
    if kind == "sigmoid":
        return torch.sigmoid(x)
    if kind == "tanh":
        return torch.tanh(x)
    if kind == "elu":
        return F.elu(x)
    if kind == "leaky_relu":
        return F.leaky_relu(x, 0.01)
    if kind == "silu":
        return F.silu(x)
    raise ValueError(f"unknown activation {kind!r}")


# ---------------------------------------------------------------------------
# fused logsoftmax + cross-entropy (reference loss_ops.cu:76,150)
# ---------------------------------------------------------------------------


class _SoftmaxXent(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, targets):
        ext = _C.ext()
        loss, lse = ext.ce_fwd(logits, targets)
        ctx.save_for_backward(logits, targets, lse)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        logits, targets, lse = ctx.saved_tensors
        ext = _C.ext()
        dlogits = ext.ce_bwd(logits, targets, lse, dloss.contiguous())
        return dlogits, None


def softmax_cross_entropy(logits: torch.Tensor, targets: torch.Tensor) -> torch.Tensor:
    """Mean cross-entropy from raw logits; ``targets`` are int64 class ids."""
    l2 = logits.reshape(-1, logits.shape[-1])
    t = targets.reshape(-1)
    if _use_hip(logits):
        per = _SoftmaxXent.apply(l2.contiguous(), t.contiguous())
        return per.mean()
    return F.cross_entropy(l2.float(), t)


# ---------------------------------------------------------------------------
# layer norm (reference layer_norm_ops.cu:21,51)
# ---------------------------------------------------------------------------


class _LayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        ext = _C.ext()
        y, mean, invstd = ext.ln_fwd(x, gamma, beta, eps)
        ctx.save_for_backward(x, gamma, mean, invstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, mean, invstd = ctx.saved_tensors
        ext = _C.ext()
        dx, dgamma, dbeta = ext.ln_bwd(x, dy.contiguous(), gamma, mean, invstd)
        return dx, dgamma, dbeta, None


class _LayerNormRes(torch.autograd.Function):
    """LayerNorm with a residual PASSTHROUGH output: ``y, xr = f(x)`` where
    xr aliases x. A pre-LN transformer block routes its residual branch
    through xr, so x has ONE consumer and the junction's grad join
    (d_x = ln_grad + d_residual) happens inside the ln_bwd kernel instead
    of an autograd fan-in add pass (2 activation-sized adds per block per
    step without this)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        ext = _C.ext()
        y, mean, invstd = ext.ln_fwd(x, gamma, beta, eps)
        ctx.save_for_backward(x, gamma, mean, invstd)
        ctx.set_materialize_grads(False)
        return y, x.view_as(x)

    @staticmethod
    def backward(ctx, dy, dres):
        x, gamma, mean, invstd = ctx.saved_tensors
        ext = _C.ext()
        if dy is None:  # residual-only consumer (degenerate use)
            return dres, None, None, None
        if dres is not None:
            dres = dres.contiguous()
        dx, dgamma, dbeta = ext.ln_bwd(x, dy.contiguous(), gamma, mean,
                                       invstd, resid=dres)
        return dx, dgamma, dbeta, None


def layer_norm_res(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor,
                   eps: float = 1e-5):
    """(layer_norm(x), residual passthrough of x) — see _LayerNormRes."""
    if _use_hip(x):
        lead = x.shape[:-1]
        y, xr = _LayerNormRes.apply(
            x.reshape(-1, x.shape[-1]).contiguous(), gamma, beta, eps)
        return (y.reshape(*lead, x.shape[-1]),
                xr.reshape(*lead, x.shape[-1]))
    return layer_norm(x, gamma, beta, eps), x


def layer_norm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor,
               eps: float = 1e-5) -> torch.Tensor:
    if _use_hip(x):
        lead = x.shape[:-1]
        y = _LayerNorm.apply(x.reshape(-1, x.shape[-1]).contiguous(), gamma, beta, eps)
        return y.reshape(*lead, x.shape[-1])
    xf = x.float()
    y = F.layer_norm(xf, (x.shape[-1],), gamma.float(), beta.float(), eps)
    return y.to(x.dtype)


# ---------------------------------------------------------------------------
# group norm NHWC (reference groupnorm_ops.cu:46-171)
# ---------------------------------------------------------------------------


class _GroupNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, groups, eps):
        ext = _C.ext()
        y, mean, invstd = ext.gn_fwd(x, gamma, beta, groups, eps)
        ctx.save_for_backward(x, gamma, mean, invstd)
        ctx.groups = groups
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, mean, invstd = ctx.saved_tensors
        ext = _C.ext()
        dx, dgamma, dbeta = ext.gn_bwd(x, dy.contiguous(), mean, invstd,
                                       gamma, ctx.groups)
        return dx, dgamma, dbeta, None, None


def group_norm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor,
               groups: int, eps: float = 1e-5) -> torch.Tensor:
    """GroupNorm over channels-last [N, ..., C]; fp32 stats, fp32 gamma/beta."""
    if _use_hip(x):
        return _GroupNorm.apply(x.contiguous(), gamma, beta, groups, eps)
    n, c = x.shape[0], x.shape[-1]
    xf = x.float().reshape(n, -1, groups, c // groups)
    mean = xf.mean(dim=(1, 3), keepdim=True)
    var = xf.var(dim=(1, 3), unbiased=False, keepdim=True)
    xhat = ((xf - mean) / torch.sqrt(var + eps)).reshape(*x.shape)
    return (xhat * gamma.float() + beta.float()).to(x.dtype)


# ---------------------------------------------------------------------------
# pointwise regression losses (reference loss_ops.cu:308-390)
# ---------------------------------------------------------------------------

PT_LOSS_KINDS = {"mse": 0, "mae": 1, "huber": 2}


class _PtLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, kind, delta):
        ext = _C.ext()
        loss = ext.ptloss_fwd(pred, target, PT_LOSS_KINDS[kind], delta)
        ctx.save_for_backward(pred, target)
        ctx.kind, ctx.delta = kind, delta
        return loss

    @staticmethod
    def backward(ctx, dloss):
        pred, target = ctx.saved_tensors
        ext = _C.ext()
        dpred = ext.ptloss_bwd(pred, target, dloss.contiguous().float(),
                               PT_LOSS_KINDS[ctx.kind], ctx.delta)
        return dpred, None, None, None


def pointwise_loss(pred: torch.Tensor, target: torch.Tensor, kind: str,
                   delta: float = 1.0) -> torch.Tensor:
    """Mean MSE / MAE / Huber loss with a fused reduce on GPU."""
    if _use_hip(pred):
        return _PtLoss.apply(pred.contiguous(),
                             target.to(pred.dtype).contiguous(), kind, delta)
    if kind == "mse":
        return F.mse_loss(pred.float(), target.float())
    if kind == "mae":
        return F.l1_loss(pred.float(), target.float())
    return F.huber_loss(pred.float(), target.float(), delta=delta)


# ---------------------------------------------------------------------------
# embedding (reference embedding_ops.cu:17,48)
# ---------------------------------------------------------------------------


class _Embedding(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ids, table):
        ext = _C.ext()
        y = ext.embedding_fwd(ids, table)
        ctx.save_for_backward(ids)
        ctx.rows = table.shape[0]
        ctx.dtype = table.dtype
        return y

    @staticmethod
    def backward(ctx, dy):
        (ids,) = ctx.saved_tensors
        ext = _C.ext()
        dtab = ext.embedding_bwd(ids, dy.contiguous(), ctx.rows)
        return None, dtab.to(ctx.dtype)


def embedding(ids: torch.Tensor, table: torch.Tensor) -> torch.Tensor:
    if _use_hip(table):
        return _Embedding.apply(ids.contiguous(), table.contiguous())
    return F.embedding(ids, table)


# ---------------------------------------------------------------------------
# scaled-dot-product attention (flash kernel on GPU, Phase 3;
# reference src/nn/blocks_impl/cuda/cudnn_flash_attention_ops.cu:81)
# ---------------------------------------------------------------------------


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
              causal: bool = True) -> torch.Tensor:
    """q/k/v: [B, H, S, D] -> [B, H, S, D]."""
    if _use_hip(q):
        from .flash import flash_attention
        return flash_attention(q, k, v, causal=causal)
    scale = q.shape[-1] ** -0.5
    s = (q.float() @ k.float().transpose(-1, -2)) * scale
    if causal:
        S = q.shape[-2]
        mask = torch.ones(S, S, dtype=torch.bool, device=q.device).triu(1)
        s = s.masked_fill(mask, float("-inf"))
    p = F.softmax(s, dim=-1)
    return (p @ v.float()).to(q.dtype)


def sdpa_materialized(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                      causal: bool = True, qoff: int = 0) -> torch.Tensor:
    """Reference-AttentionBlock math with the S x S scores materialized:
    batched MFMA GEMMs + one fused scale/causal-mask softmax pass on GPU
    (reference attention_block.cpp:144-147, cuda/softmax.cu:47-79,
    causal_mask.cu:13). q [*, M, D], k/v [*, T, D]; with ``qoff`` the
    suffix-causal offset (kv_len - M) for KV-cache prefill."""
    scale = q.shape[-1] ** -0.5
    if _use_hip(q):
        scores = matmul(q, k.transpose(-1, -2))
        p = scaled_softmax(scores, scale, causal=causal, qoff=qoff)
        return matmul(p, v)
    s = (q.float() @ k.float().transpose(-1, -2))
    p = scaled_softmax(s, scale, causal=causal, qoff=qoff)
    return (p @ v.float()).to(q.dtype)


def attention_decode(q: torch.Tensor, k_cache: torch.Tensor,
                     v_cache: torch.Tensor, pos: Optional[torch.Tensor],
                     length: int, scale: float) -> torch.Tensor:
    """Fused single-token decode attention (inference only): q [BH, D]
    against the full KV cache buffers [BH, cap, D]; live length from the
    device ``pos`` tensor (len = pos+1, hipGraph-capturable) or ``length``."""
    ext = _C.ext()
    return ext.attn_decode(q.contiguous(), k_cache, v_cache, pos,
                           length, scale)


def kv_append(k_cache: torch.Tensor, v_cache: torch.Tensor,
              k_new: torch.Tensor, v_new: torch.Tensor,
              pos: torch.Tensor) -> None:
    """Write sequence b's new K/V rows (``[B,H,1,D]``) into the
    ``[B,H,cap,D]`` caches at ``pos[b]`` (int64 ``[B]``, each < cap), in
    place: one fused launch on GPU, an index_put on CPU."""
    if _use_hip(k_cache):
        _C.ext().kv_append(k_cache, v_cache, k_new, v_new, pos)
        return
    rows = torch.arange(k_cache.shape[0], device=k_cache.device)
    k_cache[rows, :, pos] = k_new[:, :, 0]
    v_cache[rows, :, pos] = v_new[:, :, 0]


def _extend_extent(pos: torch.Tensor, n_new: Optional[torch.Tensor],
                   T: int, cap: int):
    """(p0, n) of the extend rule: p0 = pos clamped into [0, cap], n =
    n_new (T when absent) clamped into [0, min(T, cap - p0)]."""
    p0 = pos.clamp(0, cap)
    n = torch.full_like(p0, T) if n_new is None else n_new.clamp(min=0)
    return p0, torch.minimum(n, (cap - p0).clamp(max=T))


def attention_extend(q: torch.Tensor, k_cache: torch.Tensor,
                     v_cache: torch.Tensor, pos: torch.Tensor,
                     n_new: Optional[torch.Tensor] = None,
                     scale: Optional[float] = None,
                     kv_splits: int = 0) -> torch.Tensor:
    """Attention of T new query rows per sequence against that sequence's
    own cache prefix (inference only). q ``[B,H,T,D]`` (unit d-stride; the
    head slices of a merged projection are fine), caches ``[B,H,cap,D]``
    with the new rows already appended, ``pos`` / ``n_new`` int64 ``[B]``
    on the caches' device. Row ``i < n_new[b]`` of sequence b sits at
    position ``pos[b] + i`` and sees keys ``j <= pos[b] + i``; rows
    ``>= n_new[b]`` come back zero; cache slots ``>= pos[b] + n_new[b]``
    never enter the result, whatever they hold. Returns ``[B,H,T,D]`` laid
    out ``[B,T,H,D]``, so ``o.transpose(1, 2)`` is contiguous. CUDA bf16
    with D in {64, 128} runs the flash extend kernel; everything else the
    torch form of the same rule. ``kv_splits >= 1`` (T <= 16, at most 16)
    runs the kernel's split-KV form with that many blocks per (b, h) over
    the live prefix; the torch form ignores it."""
    B, H, T, D = q.shape
    cap = k_cache.shape[2]
    if scale is None:
        scale = D ** -0.5
    if q.is_cuda and q.dtype == torch.bfloat16 and D in (64, 128):
        return _C.ext().attn_extend(q, k_cache, v_cache, pos, n_new, scale,
                                    kv_splits)
    p0, n = _extend_extent(pos, n_new, T, cap)
    i = torch.arange(T, device=q.device)
    j = torch.arange(cap, device=q.device)
    live_k = j[None, :] < (p0 + n)[:, None]                       # [B, cap]
    vis = (j[None, None, :] <= (p0[:, None] + i[None, :])[:, :, None]) \
        & live_k[:, None, :]                                      # [B, T, cap]
    live_q = i[None, :] < n[:, None]                              # [B, T]
    s = (q.float() @ k_cache.float().transpose(-1, -2)) * scale
    s = s.masked_fill(~vis[:, None], float("-inf"))
    p = torch.softmax(s, dim=-1)
    p = torch.where(live_q[:, None, :, None], p, torch.zeros_like(p))
    v = torch.where(live_k[:, None, :, None], v_cache.float(),
                    torch.zeros((), device=q.device))
    o = torch.empty(B, T, H, D, dtype=q.dtype, device=q.device)
    o = o.permute(0, 2, 1, 3)
    o.copy_(p @ v)
    return o


def kv_append_n(k_cache: torch.Tensor, v_cache: torch.Tensor,
                k_new: torch.Tensor, v_new: torch.Tensor, pos: torch.Tensor,
                n_new: Optional[torch.Tensor] = None) -> None:
    """Write sequence b's new K/V rows ``i < n_new[b]`` (all T when absent)
    of ``[B,H,T,D]`` into the ``[B,H,cap,D]`` caches at slot ``pos[b] +
    i``, in place. Rows that would land at ``>= cap`` and every row of a
    negative ``pos[b]`` are dropped. One launch on GPU (fp32 / bf16), an
    index_put elsewhere."""
    if k_cache.is_cuda and k_cache.dtype in (torch.float32, torch.bfloat16):
        _C.ext().kv_append_n(k_cache, v_cache, k_new, v_new, pos, n_new)
        return
    T, cap = k_new.shape[2], k_cache.shape[2]
    i = torch.arange(T, device=k_cache.device)
    slot = pos[:, None] + i[None, :]                               # [B, T]
    n = torch.full_like(pos, T) if n_new is None else n_new
    ok = (pos[:, None] >= 0) & (i[None, :] < n[:, None]) & (slot < cap)
    bi, ti = ok.nonzero(as_tuple=True)
    k_cache[bi, :, slot[bi, ti]] = k_new[bi, :, ti]
    v_cache[bi, :, slot[bi, ti]] = v_new[bi, :, ti]


# ---------------------------------------------------------------------------
# sampling (temperature / top-k / top-p)
# ---------------------------------------------------------------------------


def _sample_rules(logits: torch.Tensor, temperature: float, top_k: int,
                  top_p: float):
    """The kept set and the unnormalised float64 weights exp(z - max) of
    every row under the sampling rules of :func:`sample_logits` (weights
    of dropped tokens are zero). Returns ``(keep [R,V] bool, w [R,V])``."""
    z = logits.double() / temperature
    V = z.shape[-1]
    keep = torch.ones_like(z, dtype=torch.bool)
    if 0 < top_k < V:
        t_k = z.topk(top_k, dim=-1).values[..., -1:]
        keep = z >= t_k
    w = torch.exp(z - z.max(dim=-1, keepdim=True).values) * keep
    if top_p < 1.0:
        p = w / w.sum(-1, keepdim=True)
        zs, order = z.sort(dim=-1, descending=True)
        c = p.gather(-1, order).cumsum(-1)
        # mass({z >= v}) is the running sum at the END of v's run of ties
        last = torch.ones_like(keep)
        last[..., :-1] = zs[..., :-1] != zs[..., 1:]
        ok = last & (c >= top_p)
        idx = torch.arange(V, device=z.device).expand_as(z)
        first = torch.where(ok, idx, V - 1).min(-1, keepdim=True).values
        t_p = zs.gather(-1, first)
        keep = keep & (z >= t_p)
        w = w * keep
    return keep, w


def sample_logits(logits: torch.Tensor, temperature: float = 1.0,
                  top_k: int = 0, top_p: float = 1.0, seed: int = 0,
                  step: Optional[torch.Tensor] = None,
                  u: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Sample one token id per row of ``logits [R,V]`` -> int64 ``[R]``.

    1. ``z = logits / temperature``; ``temperature == 0`` or ``top_k == 1``
       is greedy and returns the lowest index among the maxima.
    2. ``top_k > 0`` keeps ``{z >= t_k}``, ``t_k`` the k-th largest value.
       Ties at the threshold are all kept (bf16 logits tie constantly, and
       this is the only scan-order-independent definition).
    3. ``top_p < 1`` keeps, among the survivors with their renormalised
       probabilities, ``{z >= t_p}`` where ``t_p`` is the largest value
       with ``mass({z >= t_p}) >= top_p``; ties included again.
    4. With ``u`` in (0, 1], return the first kept index in token order
       whose running sum of kept ``exp(z - max)`` reaches ``u * total``
       (the last kept index if rounding leaves none).

    ``seed`` (host int) and ``step`` (int64 ``[1]`` tensor) select the
    random number; the result is a pure function of the arguments. ``u``
    (float ``[R]``) overrides the generator and exists for tests.

    bf16 logits on GPU run the fused HIP kernel (Philox keyed by ``seed``
    with counter ``(step, row)``; ``step`` lives on the device so a
    captured graph draws fresh numbers each replay). Everything else runs
    the float64 torch form of the same rules, drawing ``u`` from a
    ``torch.Generator`` seeded by ``(seed, step)``. The two random
    streams differ: the same seed gives different tokens on CPU and GPU.
    """
    if temperature < 0 or top_k < 0 or not (0.0 < top_p <= 1.0):
        raise ValueError("sample_logits wants temperature >= 0, top_k >= 0 "
                         "and top_p in (0, 1]")
    assert logits.dim() == 2, "sample_logits wants [R, V] logits"
    if _use_hip(logits) and logits.dtype == torch.bfloat16:
        if step is None:
            step = torch.zeros(1, dtype=torch.int64, device=logits.device)
        return _C.ext().sample_logits(logits.contiguous(), float(temperature),
                                      int(top_k), float(top_p), int(seed),
                                      step, u)
    R, V = logits.shape
    idx = torch.arange(V, device=logits.device).expand(R, V)
    if temperature == 0 or top_k == 1:
        z = logits.double()
        top = z == z.max(dim=-1, keepdim=True).values
        return torch.where(top, idx, V).min(-1).values
    keep, w = _sample_rules(logits, temperature, top_k, top_p)
    if u is None:
        st = 0 if step is None else int(step.reshape(-1)[0].item())
        g = torch.Generator().manual_seed(
            (int(seed) * 1000003 + st) % (2 ** 63))
        # (0, 1], like the device generator
        u = 1.0 - torch.rand(R, generator=g, dtype=torch.float64)
    cdf = w.cumsum(-1)
    target = u.to(device=logits.device, dtype=torch.float64).reshape(R, 1) \
        * cdf[:, -1:]
    hit = keep & (cdf >= target)
    first = torch.where(hit, idx, V).min(-1).values
    last_kept = torch.where(keep, idx, -1).max(-1).values
    return torch.where(first < V, first, last_kept)


# ---------------------------------------------------------------------------
# global gradient norm (the optimizers' clipping kernels, for logging)
# ---------------------------------------------------------------------------

def grad_global_norm(tensors) -> torch.Tensor:
    """``sqrt(sum_i ||t_i||^2)`` over a list of tensors as a 0-dim fp32
    tensor on their device, without a host sync.

    On GPU this is the multi-tensor sum-of-squares kernel plus the
    fixed-order finalize the optimizers use for ``max_grad_norm`` (fp32 and
    bf16 read in place, anything else through a contiguous copy), so the
    result is bitwise reproducible. On CPU it is the float64 torch form.
    None entries are ignored.
    """
    tensors = [t.detach() for t in tensors if t is not None]
    if _use_hip(*tensors):
        from ..nn.optim import _GradNormWorkspace, _CLIP_NORM
        dev = next(t.device for t in tensors if t.is_cuda)
        ws = _GradNormWorkspace()
        records = ws.loose_records(list(enumerate(tensors)), dev)
        state = ws.run(_C.ext(), records, dev, 0.0, count_skips=False)
        return state[_CLIP_NORM]
    sumsq = torch.zeros((), dtype=torch.float64)
    for t in tensors:
        sumsq += t.double().pow(2).sum()
    return sumsq.sqrt().float()
