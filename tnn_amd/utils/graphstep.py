"""hipGraph capture for fixed-shape inference (HIP graphs are the MI355X
answer to launch-bound serving loops; torch.cuda.CUDAGraph is hipGraph on
ROCm).

``GraphedInference`` captures one eval-mode forward over static buffers
and replays it per call — every kernel launch in the model collapses into
a single graph launch. Restricted to inference on purpose: the training
step contains host-side RNG seeding (dropout) and python-side Adam step
counts that a captured graph would freeze (documented round-2 work).
"""

from __future__ import annotations


import torch


class GraphedInference:
    def __init__(self, model: torch.nn.Module, example_input: torch.Tensor,
                 warmup: int = 3):
        assert example_input.is_cuda, "graph capture needs GPU tensors"
        self.model = model
        model.eval()
        self.static_in = example_input.clone()
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            with torch.no_grad():
                for _ in range(warmup):
                    out = model(self.static_in)
        torch.cuda.current_stream().wait_stream(stream)
        self.graph = torch.cuda.CUDAGraph()
        with torch.no_grad():
            with torch.cuda.graph(self.graph):
                self.static_out = model(self.static_in)

    @torch.no_grad()
    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        self.static_in.copy_(x)
        self.graph.replay()
        return self.static_out


# two runs of unwritten gradients closer than this many elements are zeroed
# with one fill: refilling a few written elements in between (their sink
# overwrites them later in the step) costs less than another launch
ZERO_MERGE_GAP = 16384


def unwritten_runs(layout, written, merge_gap: int = ZERO_MERGE_GAP):
    """``[(start, end)]`` element ranges of one gradient slab that a step
    must zero: every parameter of ``layout`` (``[(key, offset, numel)]`` in
    slab order) whose key is not in ``written``, adjacent ranges joined, and
    ranges at most ``merge_gap`` elements apart joined across the gap."""
    runs = []
    for key, off, numel in layout:
        if key in written or numel == 0:
            continue
        if runs and off - runs[-1][1] <= merge_gap:
            runs[-1][1] = off + numel
        else:
            runs.append([off, off + numel])
    return [(a, b) for a, b in runs]


class GraphedTrainStep:
    """Whole-training-step hipGraph capture: grad-zeroing, forward, loss,
    backward and the fused optimizer update replay as ONE graph launch
    (the round-1 blockers are solved device-side: dropout Philox streams
    combine a capture-baked salt with an in-graph device counter, and the
    Adam bias correction reads the same counter instead of a baked-in
    host step — csrc/optim.hip, elementwise.hip, batchnorm.hip).

    The learning rate lives on the device too: the update kernels read
    ``lr_dev``, and ``__call__`` refreshes it (one fill on the stream,
    outside the graph, no sync) whenever ``optimizer.lr`` has changed, so a
    scheduler stepped between calls takes effect. Gradient clipping
    (``max_grad_norm``) needs nothing special: its two launches are
    captured with the rest.

    Gradients are written once: the slab views are registered as gradient
    sinks (``ops.functional.GradSinks``), so the conv and batch-norm
    backwards reduce straight into ``p.grad`` instead of handing autograd a
    tensor to add to a zeroed one. The first warm-up step zeroes the whole
    slabs and learns which parameters the sinks wrote; every later step
    zeroes only the others (unused parameters, layers that return their
    gradient the old way), which must still see a zero gradient.
    ``TNN_GRAD_SINK=0`` turns this off.

    Constraints: fixed shapes, the optimizer's python ``step_count`` stays
    at its capture value (the device counter is the truth; checkpoint via
    ``sync_step_count()``).
    """

    def __init__(self, model, criterion, optimizer, example_x, example_y,
                 warmup: int = 3):
        from ..ops.functional import (GradSinks, grad_sinks_enabled,
                                      set_graph_seed_ctr, set_grad_sinks)
        assert example_x.is_cuda
        self.model, self.criterion, self.optimizer = model, criterion, optimizer
        self.static_x = example_x.clone()
        self.static_y = example_y.clone()
        dev = example_x.device
        self.step_ctr = torch.zeros(1, dtype=torch.int64, device=dev)
        model.train()
        optimizer._step_dev = self.step_ctr
        self.lr_dev = torch.full((1,), float(optimizer.lr),
                                 dtype=torch.float32, device=dev)
        self._lr_written = optimizer.lr
        optimizer._lr_dev = self.lr_dev
        # pack all grads into per-dtype slabs (the reference GraphContext's
        # grad-slab idea): grad zeroing is then ONE fill per dtype instead
        # of a launch per parameter (torch._foreach_zero_ fell back to
        # per-tensor fills on ROCm — ~34 launches/step on WRN)
        groups = {}
        for prm in optimizer.params:
            groups.setdefault(prm.dtype, []).append(prm)
        self._grad_slabs = []
        self._slab_layout = []   # per slab: [(param key, offset, numel)]
        for dt, ps in groups.items():
            slab = torch.zeros(sum(pp.numel() for pp in ps), dtype=dt,
                               device=dev)
            off = 0
            layout = []
            for pp in ps:
                pp.grad = slab[off:off + pp.numel()].view_as(pp)
                layout.append((pp.data_ptr(), off, pp.numel()))
                off += pp.numel()
            self._grad_slabs.append(slab)
            self._slab_layout.append(layout)
        self._sinks = (GradSinks(optimizer.params) if grad_sinks_enabled()
                       else None)
        self._sink_written = None   # learnt in the first step
        self._zero_views = None     # None: fill the whole slabs
        set_graph_seed_ctr(self.step_ctr)
        set_grad_sinks(self._sinks)
        try:
            stream = torch.cuda.Stream()
            stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(stream):
                for _ in range(warmup):
                    self._step_body()
            torch.cuda.current_stream().wait_stream(stream)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self.static_loss = self._step_body()
        finally:
            set_graph_seed_ctr(None)
            set_grad_sinks(None)

    def _step_body(self):
        self.step_ctr.add_(1)
        # grads are views of the packed slabs: one fill per dtype, or, once
        # the sink-written set is known, one per run of parameters outside it
        if self._sinks is not None:
            self._sinks.begin_step()
        if self._zero_views is None:
            for slab in self._grad_slabs:
                slab.zero_()
        else:
            for v in self._zero_views:
                v.zero_()
        out = self.model(self.static_x)
        loss = self.criterion(out, self.static_y)
        loss.backward()
        if self._sinks is not None:
            written = frozenset(self._sinks.written)
            if self._sink_written is None:
                self._sink_written = written
                self._zero_views = [
                    slab[a:b]
                    for slab, layout in zip(self._grad_slabs,
                                            self._slab_layout)
                    for a, b in unwritten_runs(layout, written)]
            else:
                assert written == self._sink_written, (
                    "the gradient sinks wrote another set of parameters than "
                    "in the first step; the zeroing plan no longer holds")
        self.optimizer.step()
        return loss

    def __call__(self, x=None, y=None) -> torch.Tensor:
        """Run one training step; returns the (device) loss tensor."""
        if x is not None:
            self.static_x.copy_(x)
        if y is not None:
            self.static_y.copy_(y)
        if self.optimizer.lr != self._lr_written:
            self.lr_dev.fill_(float(self.optimizer.lr))
            self._lr_written = self.optimizer.lr
        self.graph.replay()
        return self.static_loss

    def sync_step_count(self):
        """Pull the device step counter back into the optimizer (one host
        sync; call before checkpointing)."""
        self.optimizer.step_count = int(self.step_ctr.item())
