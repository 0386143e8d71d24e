"""Optimizers with fused CDNA4 update kernels
(reference include/nn/optimizers.hpp:70,149; GPU kernels
src/nn/optimizers_impl/cuda/sgd_kernels.cu:17, adam_kernels.cu:19).

Low-precision params (bf16) automatically get an fp32 master copy in
optimizer state; the fused kernel updates the master and writes the cast
parameter in the same pass (the reference trains fp32 only — this is the
MI355X-native mixed-precision upgrade).

Global-norm gradient clipping (``max_grad_norm > 0``) is fused into the
same kernels: one multi-tensor sum-of-squares launch per grad dtype, a
one-block finalize that leaves ``{sumsq, norm, coef, skip}`` on the device,
and update kernels that scale the gradient by ``coef`` as they read it
(the gradients themselves are not modified). The rule is
``torch.nn.utils.clip_grad_norm_``'s: ``coef = min(1, max_norm / (norm +
1e-6))``. A step whose norm is not finite changes nothing — parameters,
master copies, moments and momentum stay bit-identical — and is counted
in ``skipped_steps()``. ``step_count`` (and the device step counter of a
graph-captured step) still advances on a skipped step, so eager and
captured training stay identical and the dropout counter keeps moving.
"""

from __future__ import annotations

import math
from typing import Any, Callable, Dict, Iterable, List, Optional

import torch

from .. import _C

_MT_CHUNK = 16384  # MT_CHUNK in optim.hip
_DT_CODE = {torch.float32: 0, torch.bfloat16: 1}
# slots of the device clip state vector (ClipSlot in kernels.h)
_CLIP_SUMSQ, _CLIP_NORM, _CLIP_COEF, _CLIP_SKIP, _CLIP_STATE = 0, 1, 2, 3, 4

_SKIP = object()  # CPU path: the global norm was not finite


def _chunk_map(numels, dev) -> torch.Tensor:
    """Block -> (tensor_idx << 32 | chunk) over MT_CHUNK-element spans."""
    chunks = []
    for ti, n in enumerate(numels):
        for c in range((n + _MT_CHUNK - 1) // _MT_CHUNK):
            chunks.append((ti << 32) | c)
    return torch.tensor(chunks, dtype=torch.int64, device=dev)


class _GradNormWorkspace:
    """Device buffers and descriptor caches of the global gradient norm.
    Everything is allocated on first use and reused while the gradient
    pointers stay the same, so a warmed-up step allocates nothing (hipGraph
    capture) and uploads no descriptor."""

    def __init__(self):
        self.chunks: Dict[Any, torch.Tensor] = {}
        self.descs: Dict[Any, Any] = {}
        self.stage: Dict[Any, torch.Tensor] = {}
        self.part: Optional[torch.Tensor] = None
        self.state: Optional[torch.Tensor] = None
        self.skipped: Optional[torch.Tensor] = None

    def loose_records(self, keyed_grads, dev):
        """Launch records (2-wide ``[grad ptr, numel]`` descriptors, one per
        grad dtype) for gradients outside a multi-tensor Adam group. The
        rare non-contiguous or non-fp32/bf16 gradient is read through a
        contiguous staging copy kept per ``key``."""
        by_dt: Dict[torch.dtype, List[torch.Tensor]] = {}
        for key, g in keyed_grads:
            if g.dtype not in _DT_CODE or not g.is_contiguous():
                dt = g.dtype if g.dtype in _DT_CODE else torch.float32
                buf = self.stage.get(key)
                if (buf is None or buf.shape != g.shape or buf.dtype != dt
                        or buf.device != g.device):
                    buf = torch.empty(g.shape, dtype=dt, device=g.device)
                    self.stage[key] = buf
                buf.copy_(g)
                g = buf
            by_dt.setdefault(g.dtype, []).append(g)
        records = []
        for dt, gs in by_dt.items():
            numels = tuple(g.numel() for g in gs)
            chunks_t = self.chunks.get(numels)
            if chunks_t is None:
                chunks_t = self.chunks[numels] = _chunk_map(numels, dev)
            desc = []
            for g in gs:
                desc += [g.data_ptr(), g.numel()]
            dkey = tuple(desc)
            ent = self.descs.get((dt, numels))
            if ent is not None and ent[0] == dkey:
                desc_t = ent[1]
            else:
                desc_t = torch.tensor(desc, dtype=torch.int64, device=dev)
                self.descs[(dt, numels)] = (dkey, desc_t)
            records.append((desc_t, chunks_t, 2, 0, 1, _DT_CODE[dt]))
        return records

    def run(self, ext, records, dev, max_norm: float,
            norm_reduce: Optional[Callable] = None,
            count_skips: bool = True) -> torch.Tensor:
        """Launch the sum-of-squares kernels of ``records`` — tuples
        ``(desc, chunks, stride, grad slot, numel slot, dtype code)`` — and
        the finalize; returns the device state vector."""
        total = sum(r[1].numel() for r in records)
        if self.state is None or self.state.device != dev:
            self.state = torch.zeros(_CLIP_STATE, dtype=torch.float32,
                                     device=dev)
            self.skipped = torch.zeros(1, dtype=torch.int64, device=dev)
            self.part = None
        if self.part is None or self.part.numel() < total:
            self.part = torch.empty(max(total, 1), dtype=torch.float32,
                                    device=dev)
        base = 0
        for desc_t, chunks_t, stride, gslot, nslot, dt in records:
            if chunks_t.numel():
                ext.grad_sumsq_mt(desc_t, chunks_t, stride, gslot, nslot, dt,
                                  self.part, base)
            base += chunks_t.numel()
        skipped = self.skipped if count_skips else None
        if norm_reduce is None:
            ext.clip_finalize(self.part, total, max_norm, self.state,
                              skipped=skipped)
        else:
            # parameters are spread over ranks: fold the local partials,
            # sum the one-element sumsq across ranks, derive the scalars
            # from the global value (every rank gets the same coef / skip)
            ext.clip_finalize(self.part, total, max_norm, self.state)
            sumsq = self.state[_CLIP_SUMSQ:_CLIP_SUMSQ + 1]
            norm_reduce(sumsq)
            ext.clip_finalize(self.part, 0, max_norm, self.state,
                              skipped=skipped, sumsq_in=sumsq)
        return self.state


class Optimizer:
    _type = "optimizer"

    def __init__(self, params: Iterable[torch.nn.Parameter], lr: float,
                 max_grad_norm: float = 0.0):
        self.params: List[torch.nn.Parameter] = [p for p in params if p.requires_grad]
        self.lr = lr
        if max_grad_norm < 0:
            raise ValueError("max_grad_norm must be >= 0 (0 disables clipping)")
        self.max_grad_norm = float(max_grad_norm)
        self.state: Dict[int, Dict[str, Any]] = {}
        self.step_count = 0
        # device step counter / learning rate for hipGraph-captured steps
        # (read on device instead of baked in at capture)
        self._step_dev = None
        self._lr_dev = None
        # Hook ``f(sumsq)`` that sums the one-element fp32 tensor in place
        # over the ranks that hold the other parameters. PipelineEngine
        # installs it (stages own disjoint parameters). Data-parallel
        # training needs none: after the bucketed gradient all-reduce every
        # rank holds identical gradients, so the local norm is the global one.
        self.norm_reduce: Optional[Callable[[torch.Tensor], Any]] = None
        self._gn: Optional[_GradNormWorkspace] = None
        self._last_norm: Optional[torch.Tensor] = None
        self._skipped_host = 0

    def zero_grad(self):
        for p in self.params:
            p.grad = None

    # -- global-norm clipping -------------------------------------------------
    @property
    def last_grad_norm(self) -> Optional[torch.Tensor]:
        """Pre-clip global gradient norm of the latest step as a 0-dim
        tensor on the parameters' device (no host sync); None before the
        first clipped step."""
        return self._last_norm

    def skipped_steps(self) -> int:
        """Number of steps skipped for a non-finite norm (one host sync)."""
        n = self._skipped_host
        if self._gn is not None and self._gn.skipped is not None:
            n += int(self._gn.skipped.item())
        return n

    def _workspace(self) -> _GradNormWorkspace:
        if self._gn is None:
            self._gn = _GradNormWorkspace()
        return self._gn

    def _clip_cpu(self, grads):
        """torch form of the kernels' rule, float64 norm. Returns the
        coefficient, or ``_SKIP`` when the norm is not finite."""
        sumsq = torch.zeros((), dtype=torch.float64)
        for g in grads:
            sumsq += g.detach().double().pow(2).sum()
        if self.norm_reduce is not None:
            t = sumsq.float().reshape(1)
            self.norm_reduce(t)
            sumsq = t[0].double()
        norm = float(sumsq.sqrt())
        self._last_norm = torch.tensor(norm, dtype=torch.float32)
        if not math.isfinite(norm):
            self._skipped_host += 1
            return _SKIP
        return min(1.0, self.max_grad_norm / (norm + 1e-6))

    def _clip_gpu(self, ext, records, dev) -> torch.Tensor:
        state = self._workspace().run(ext, records, dev, self.max_grad_norm,
                                      self.norm_reduce)
        self._last_norm = state[_CLIP_NORM]
        return state

    @torch.no_grad()
    def step(self):
        """One update. With ``max_grad_norm > 0`` every parameter that has
        a grad counts towards the global norm; ``step_count`` advances even
        when the step is skipped for a non-finite norm."""
        self.step_count += 1
        if not self.params:
            return
        todo = [(i, p) for i, p in enumerate(self.params)
                if p.grad is not None]
        clip = None
        if self.max_grad_norm > 0:
            if self.params[0].is_cuda:
                gn = self._workspace()
                dev = self.params[0].device
                clip = self._clip_gpu(
                    _C.ext(),
                    gn.loose_records([(i, p.grad) for i, p in todo], dev), dev)
            else:
                clip = self._clip_cpu([p.grad for _, p in todo])
                if clip is _SKIP:
                    return
        for i, p in todo:
            st = self.state.setdefault(i, {})
            if p.dtype != torch.float32 and "master" not in st:
                st["master"] = p.detach().float().clone()
            self._update(p, p.grad, st, clip)

    def _update(self, p, g, st, clip=None):
        """``clip``: the device state vector on GPU, the coefficient (a
        python float) on CPU, None without clipping."""
        raise NotImplementedError

    def get_config(self) -> Dict[str, Any]:
        return {"type": self._type, "lr": self.lr, **self.extra_config()}

    def extra_config(self) -> Dict[str, Any]:
        return self._clip_config()

    def _clip_config(self) -> Dict[str, Any]:
        # only when set: configs and checkpoints written without clipping
        # keep their exact bytes
        return ({"max_grad_norm": self.max_grad_norm}
                if self.max_grad_norm else {})

    # -- state round-trip for checkpoint/stage-redeploy ----------------------
    def state_tensors(self):
        out = []
        for i in sorted(self.state):
            for k in sorted(self.state[i]):
                v = self.state[i][k]
                if torch.is_tensor(v):
                    out.append((f"{i}.{k}", v))
        return out

    def materialize_state_slot(self, name: str):
        """Create (and return) the state tensor named ``"{param_idx}.{key}"``
        so a checkpoint can be restored into a freshly constructed optimizer
        whose lazy state dict is still empty. Returns None for names this
        optimizer cannot place (unknown key or out-of-range param index)."""
        idx_s, _, key = name.partition(".")
        try:
            i = int(idx_s)
        except ValueError:
            return None
        if not key or i < 0 or i >= len(self.params):
            return None
        p = self.params[i]
        st = self.state.setdefault(i, {})
        if key in st and torch.is_tensor(st[key]):
            return st[key]
        if key == "master":
            st[key] = p.detach().float().clone()
        elif key in ("m", "v", "buf"):
            st[key] = torch.zeros(p.shape, dtype=torch.float32, device=p.device)
        else:
            return None
        return st[key]


class SGD(Optimizer):
    _type = "sgd"

    def __init__(self, params, lr=0.01, momentum=0.0, weight_decay=0.0,
                 nesterov=False, max_grad_norm=0.0):
        super().__init__(params, lr, max_grad_norm)
        self.momentum, self.weight_decay, self.nesterov = momentum, weight_decay, nesterov

    def _update(self, p, g, st, clip=None):
        if p.is_cuda:
            ext = _C.ext()
            master = st.get("master", p.data)
            if self.momentum != 0.0 and "buf" not in st:
                st["buf"] = torch.zeros_like(master)
            if not g.is_contiguous():
                g = g.contiguous()
            ext.sgd_step(p.data, master, g, st.get("buf"),
                         self.lr, self.momentum, self.weight_decay, self.nesterov,
                         clip=clip, lr_dev=self._lr_dev)
            return
        master = st.get("master", p.data)
        gf = g.float()
        if clip is not None:
            gf = gf * clip
        if self.weight_decay:
            gf = gf.add(master, alpha=self.weight_decay)
        if self.momentum != 0.0:
            buf = st.setdefault("buf", torch.zeros_like(master))
            buf.mul_(self.momentum).add_(gf)
            gf = gf.add(buf, alpha=self.momentum) if self.nesterov else buf
        master.add_(gf, alpha=-self.lr)
        if master.data_ptr() != p.data.data_ptr():
            p.data.copy_(master)

    def extra_config(self):
        return {"momentum": self.momentum, "weight_decay": self.weight_decay,
                "nesterov": self.nesterov, **self._clip_config()}


class Adam(Optimizer):
    _type = "adam"
    _adamw = False

    def __init__(self, params, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8,
                 weight_decay=0.0, max_grad_norm=0.0):
        super().__init__(params, lr, max_grad_norm)
        self.beta1, self.beta2, self.eps, self.weight_decay = beta1, beta2, eps, weight_decay
        self._mt_chunk_cache = {}
        self._mt_desc_cache = {}

    @torch.no_grad()
    def step(self):
        """Multi-tensor fused update on GPU: one kernel launch per
        (param dtype, grad dtype, has-master) group instead of one per
        parameter (~150 launches -> ~2 on GPT-2). With ``max_grad_norm > 0``
        the norm kernel reads the same descriptors first; ``step_count``
        advances even when the step is skipped for a non-finite norm."""
        if not self.params or not self.params[0].is_cuda:
            return super().step()
        self.step_count += 1
        ext = _C.ext()
        groups = {}
        singles = []
        for i, p in enumerate(self.params):
            if p.grad is None:
                continue
            st = self.state.setdefault(i, {})
            if p.dtype != torch.float32 and "master" not in st:
                st["master"] = p.detach().float().clone()
            if "m" not in st:
                ref = st.get("master", p.data)
                st["m"] = torch.zeros_like(ref, dtype=torch.float32)
                st["v"] = torch.zeros_like(ref, dtype=torch.float32)
            g = p.grad
            if (g.dtype not in (torch.float32, torch.bfloat16)
                    or not g.is_contiguous() or g.dtype != p.dtype):
                singles.append((i, p, g, st))
                continue
            groups.setdefault((p.dtype, g.dtype, "master" in st),
                              []).append((i, p, g, st))
        launches = []
        for (pdt, gdt, has_master), items in groups.items():
            if len(items) == 1:
                singles.append(items[0])
                continue
            dev = items[0][1].device
            # chunk map depends only on the numels (stable): cache it
            numels = tuple(p.numel() for _, p, _, _ in items)
            chunks_t = self._mt_chunk_cache.get(numels)
            if chunks_t is None:
                chunks_t = _chunk_map(numels, dev)
                self._mt_chunk_cache[numels] = chunks_t
            desc = []
            for _, p, g, st in items:
                desc += [p.data_ptr(),
                         st["master"].data_ptr() if has_master else 0,
                         g.data_ptr(), st["m"].data_ptr(),
                         st["v"].data_ptr(), p.numel()]
            # pointer-stable across steps: cache the device copy per dtype
            # group, revalidated against the pointer tuple (also keeps H2D
            # pageable copies out of hipGraph capture)
            dkey = tuple(desc)
            ck = (pdt, gdt, has_master, numels)
            ent = self._mt_desc_cache.get(ck)
            if ent is not None and ent[0] == dkey:
                desc_t = ent[1]
            else:
                desc_t = torch.tensor(desc, dtype=torch.int64, device=dev)
                self._mt_desc_cache[ck] = (dkey, desc_t)
            launches.append((desc_t, chunks_t, pdt, gdt, has_master))
        clip = None
        if self.max_grad_norm > 0:
            # the 6-wide Adam descriptors are read as they are (grad pointer
            # in slot 2, numel in slot 5); what runs single-tensor gets a
            # 2-wide descriptor of its own
            dev = self.params[0].device
            records = [(desc_t, chunks_t, 6, 2, 5, _DT_CODE[gdt])
                       for desc_t, chunks_t, _, gdt, _ in launches]
            records += self._workspace().loose_records(
                [(i, g) for i, _, g, _ in singles], dev)
            clip = self._clip_gpu(ext, records, dev)
        for _, p, g, st in singles:
            self._update(p, g, st, clip)
        for desc_t, chunks_t, pdt, gdt, has_master in launches:
            ext.adam_step_mt(desc_t, chunks_t,
                             0 if pdt == torch.float32 else 1,
                             0 if gdt == torch.float32 else 1, has_master,
                             self.step_count, self.lr, self.beta1, self.beta2,
                             self.eps, self.weight_decay, self._adamw,
                             step_dev=self._step_dev, clip=clip,
                             lr_dev=self._lr_dev)

    def _update(self, p, g, st, clip=None):
        if "m" not in st:
            ref = st.get("master", p.data)
            st["m"] = torch.zeros_like(ref, dtype=torch.float32)
            st["v"] = torch.zeros_like(ref, dtype=torch.float32)
        if p.is_cuda:
            ext = _C.ext()
            master = st.get("master", p.data)
            if not g.is_contiguous():
                g = g.contiguous()
            ext.adam_step(p.data, master, g, st["m"], st["v"], self.step_count,
                          self.lr, self.beta1, self.beta2, self.eps,
                          self.weight_decay, self._adamw,
                          step_dev=self._step_dev, clip=clip,
                          lr_dev=self._lr_dev)
            return
        master = st.get("master", p.data)
        gf = g.float()
        if clip is not None:
            gf = gf * clip
        if self.weight_decay and not self._adamw:
            gf = gf.add(master, alpha=self.weight_decay)
        st["m"].mul_(self.beta1).add_(gf, alpha=1 - self.beta1)
        st["v"].mul_(self.beta2).addcmul_(gf, gf, value=1 - self.beta2)
        bc1 = 1 - self.beta1 ** self.step_count
        bc2 = 1 - self.beta2 ** self.step_count
        if self._adamw and self.weight_decay:
            master.mul_(1 - self.lr * self.weight_decay)
        denom = (st["v"] / bc2).sqrt_().add_(self.eps)
        master.addcdiv_(st["m"], denom, value=-self.lr / bc1)
        if master.data_ptr() != p.data.data_ptr():
            p.data.copy_(master)

    def extra_config(self):
        return {"beta1": self.beta1, "beta2": self.beta2, "eps": self.eps,
                "weight_decay": self.weight_decay, **self._clip_config()}


class AdamW(Adam):
    _type = "adamw"
    _adamw = True


_OPTS = {"sgd": SGD, "adam": Adam, "adamw": AdamW}


def optimizer_from_config(cfg: Dict[str, Any], params) -> Optimizer:
    cfg = dict(cfg)
    cls = _OPTS[cfg.pop("type")]
    return cls(params, **cfg)
