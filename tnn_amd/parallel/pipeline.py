"""Pipeline-parallel engine (reference include/distributed/coordinator.hpp:50,
worker.hpp:41, train.hpp:19-128 — re-designed for RCCL/xGMI).

One rank per GPU; rank r runs pipeline stage r. Differences from the
reference, on purpose:

- **Schedule**: non-interleaved 1F1B instead of the reference's semi-async
  all-forwards-then-drain (coordinator.hpp:165-223). 1F1B bounds in-flight
  activations per stage to ``num_stages - rank`` micro-batches instead of
  all of them — the micro-batch activation queues the reference keeps in
  per-``mb_id`` layer caches live here in the autograd graphs of the
  outstanding micro-batches.
- **Transport**: activations/grads are RCCL P2P device-buffer send/recv over
  xGMI (no host staging, no serialization), shapes agreed once up front via
  shape inference instead of per-message headers.
- **Control plane**: stage configs are shipped as JSON-able dicts over a
  gloo object channel (reference CONFIG_TRANSFER), and parameter updates
  are local per-rank optimizer steps after the batch drains (reference
  UPDATE_PARAMETERS barrier).
"""

from __future__ import annotations

from typing import Any, Dict, List, Optional, Tuple

import torch

from ..nn.accuracy import accuracy
from ..nn.blocks import Sequential
from ..nn.layer import layer_from_config
from ..nn.losses import Loss, CrossEntropyLoss
from ..nn.optim import Optimizer, optimizer_from_config
from ..nn.schedulers import scheduler_from_config
from ..utils.logging import get_logger
from ..utils.profiler import Profiler, EventType
from .comm import Communicator
from .partitioner import partition_model, Partitioner

log = get_logger("pipeline")


class PipelineEngine:
    def __init__(self,
                 model: Optional[Sequential],
                 comm: Communicator,
                 input_shape: Tuple[int, ...],
                 num_microbatches: int = 4,
                 criterion: Optional[Loss] = None,
                 optimizer_config: Optional[Dict[str, Any]] = None,
                 scheduler_config: Optional[Dict[str, Any]] = None,
                 partition_strategy: str = "weighted",
                 device: Optional[torch.device] = None,
                 io_dtype: torch.dtype = torch.float32,
                 sync_weights: bool = False):
        """``model`` is required on rank 0 (the coordinator role); other
        ranks receive their stage config over the control plane
        (reference deploy_stages, coordinator.hpp:368-395)."""
        self.comm = comm
        self.rank, self.world = comm.rank, comm.world_size
        self.num_stages = self.world
        self.M = num_microbatches
        self.criterion = criterion or CrossEntropyLoss()
        self.device = device or torch.device(
            "cuda" if torch.cuda.is_available() else "cpu")
        self.io_dtype = io_dtype
        self.input_shape = tuple(input_shape)

        # -- partition on rank 0, deploy configs (CONFIG_TRANSFER) ----------
        if self.rank == 0:
            assert model is not None
            stages = partition_model(model, self.num_stages, self.input_shape,
                                     partition_strategy)
            boundary = Partitioner.boundary_shapes(stages, self.input_shape)
            payload = {"configs": [s.get_config() for s in stages],
                       "boundary": boundary}
            self._rank0_stages = stages
        else:
            payload = None
        payload = comm.broadcast_object(payload, src=0)
        self.boundary = [tuple(b) for b in payload["boundary"]]
        if self.rank == 0 and model is not None:
            self.stage = self._rank0_stages[0] if self.world > 1 else model
        else:
            self.stage = layer_from_config(payload["configs"][self.rank])
        if sync_weights and self.world > 1:
            self._sync_weights()
        self.stage.to(self.device)
        if io_dtype != torch.float32:
            self._cast_stage(io_dtype)

        self.in_shape = self.boundary[self.rank]
        self.out_shape = self.boundary[self.rank + 1]
        self.is_first = self.rank == 0
        self.is_last = self.rank == self.world - 1

        # per-rank profiler (reference worker.hpp:146-204 hook points);
        # enable with engine.profiler.start(), merge via gather_profiles()
        self.profiler = Profiler(source=f"rank{self.rank}")

        opt_cfg = optimizer_config or {"type": "adamw", "lr": 1e-3}
        self.optimizer: Optimizer = optimizer_from_config(
            opt_cfg, self.stage.parameters())
        if self.world > 1:
            # stages own disjoint parameters: the clipping norm
            # (max_grad_norm) must be the global one, so the local sum of
            # squares is summed over the ranks before the coefficient and
            # the skip decision are derived — the same on every stage
            self.optimizer.norm_reduce = self.comm.allreduce_
        self.scheduler = (scheduler_from_config(scheduler_config, self.optimizer)
                          if scheduler_config else None)
        n_params = sum(p.numel() for p in self.stage.parameters())
        log.info("rank %d: stage %s with %d layers, %.2fM params, in=%s out=%s",
                 self.rank, self.stage.name, len(self.stage),
                 n_params / 1e6, self.in_shape, self.out_shape)

    # ------------------------------------------------------------------
    def _cast_stage(self, dtype):
        """Cast compute params + layer io dtypes to bf16; BN/LN affine and
        running stats stay fp32."""
        from ..nn.layer import cast_compute_dtype
        cast_compute_dtype(self.stage, dtype)

    def _sync_weights(self):
        """Ship rank-0's partitioned weights to every stage owner so all
        ranks train the exact model rank 0 built (the reference re-inits
        on workers; this also enables bitwise parity tests)."""
        sds = None
        if self.rank == 0:
            sds = [{k: v.cpu() for k, v in s.state_dict().items()}
                   for s in self._rank0_stages]
        sds = self.comm.broadcast_object(sds, src=0)
        self.stage.load_state_dict(sds[self.rank])

    # ------------------------------------------------------------------
    def _recv_act(self, mb_size: int) -> torch.Tensor:
        t = torch.empty(mb_size, *self.in_shape, device=self.device,
                        dtype=self.io_dtype)
        self.comm.recv(t, self.rank - 1)
        return t.requires_grad_(True)

    def _recv_grad(self, out: torch.Tensor) -> torch.Tensor:
        g = torch.empty_like(out)
        self.comm.recv(g, self.rank + 1)
        return g

    # ------------------------------------------------------------------
    def train_batch(self, x: Optional[torch.Tensor],
                    y: Optional[torch.Tensor],
                    step: bool = True) -> Dict[str, float]:
        """One optimizer step over a global batch split into M micro-batches.

        ``x`` is consumed on the first rank, ``y`` on the last; other ranks
        may pass None. Returns loss/accuracy stats (valid on the last rank;
        use :meth:`broadcast_stats` if every rank needs them).
        """
        self.stage.train()
        M = self.M
        if self.is_first:
            micro_x = list(x.to(self.device).chunk(M, dim=0))
            assert len(micro_x) == M, "batch not divisible into microbatches"
            mb_size = micro_x[0].shape[0]
        else:
            mb_size = (x.shape[0] if x is not None else
                       y.shape[0]) // M if (x is not None or y is not None) else None
            if mb_size is None:
                raise ValueError("non-first ranks need x or y for mb size")
        if self.is_last:
            micro_y = list(y.to(self.device).chunk(M, dim=0))

        # -- comm pattern -----------------------------------------------------
        # Warmup is forward-only traffic and cooldown backward-only (both
        # acyclic), but in the steady 1F1B phase every middle rank both
        # sends an activation to r+1 and receives a gradient from r+1 (and
        # symmetrically with r-1). Issued as separate ops those two
        # rendezvous transfers deadlock on RCCL — the send kernel occupies
        # the comm stream until the peer posts its recv, and the peer is
        # symmetrically blocked (gloo's buffering hides this on CPU). So
        # bidirectional pairs always travel as ONE batched P2P group
        # (rcclGroupStart/End), the Megatron send_forward_recv_backward /
        # send_backward_recv_forward pattern.
        import torch.distributed as dist

        fifo: List[Tuple[Optional[torch.Tensor], torch.Tensor]] = []
        losses: List[torch.Tensor] = []
        accs: List[torch.Tensor] = []
        send_works: List[Any] = []

        def forward_mb(inp, idx):
            with self.profiler.span(EventType.COMPUTE, f"forward mb{idx}"):
                out = self.stage(inp)
            if self.is_last:
                my = micro_y[idx]
                loss = self.criterion(out, my) / M
                losses.append(loss)
                with torch.no_grad():  # on-device accuracy (no .item() stall)
                    pred = out.detach().reshape(-1, out.shape[-1]).argmax(-1)
                    t = (my.reshape(-1, my.shape[-1]).argmax(-1)
                         if my.dim() == out.dim() else my.reshape(-1).long())
                    accs.append((pred == t).float().mean())
                fifo.append((inp, loss))
                return None
            fifo.append((inp, out))
            return out

        def backward_mb(grad_out, idx):
            inp, out = fifo.pop(0)
            with self.profiler.span(EventType.COMPUTE, f"backward mb{idx}"):
                if self.is_last:
                    out.backward()  # out is the micro-loss
                else:
                    torch.autograd.backward(out, grad_out)
            return None if self.is_first else inp.grad

        def recv_forward(idx):
            if self.is_first:
                mx = micro_x[idx]
                # token ids stay integral (embedding input); only float
                # inputs follow the io dtype
                return mx.to(self.io_dtype) if mx.is_floating_point() else mx
            with self.profiler.span(EventType.COMMUNICATION, f"recv_act {idx}"):
                return self._recv_act(mb_size)

        def send_forward(out):
            if out is not None:
                send_works.append(self.comm.isend(out, self.rank + 1))

        def send_fwd_recv_bwd(out):
            """Batched: ship the newest activation to r+1 and receive the
            gradient for the oldest in-flight one (same peer, one group)."""
            if self.is_last:
                return None
            grad = torch.empty_like(fifo[0][1])
            with self.profiler.span(EventType.COMMUNICATION, "send_fwd_recv_bwd"):
                reqs = self.comm.batch_p2p([
                    dist.P2POp(dist.isend, out.contiguous(), self.rank + 1),
                    dist.P2POp(dist.irecv, grad, self.rank + 1)])
                for r in reqs:
                    r.wait()
            return grad

        def send_bwd_recv_fwd(ingrad):
            """Batched: ship the input-gradient to r-1 and receive the next
            micro-batch activation from it."""
            act = torch.empty(mb_size, *self.in_shape, device=self.device,
                              dtype=self.io_dtype)
            with self.profiler.span(EventType.COMMUNICATION, "send_bwd_recv_fwd"):
                reqs = self.comm.batch_p2p([
                    dist.P2POp(dist.isend, ingrad.contiguous(), self.rank - 1),
                    dist.P2POp(dist.irecv, act, self.rank - 1)])
                for r in reqs:
                    r.wait()
            return act.requires_grad_(True)

        def send_backward(ingrad):
            if ingrad is not None:
                send_works.append(self.comm.isend(ingrad, self.rank - 1))

        warmup = min(self.num_stages - 1 - self.rank, M)
        steady = M - warmup
        fwd_idx = bwd_idx = 0

        for _ in range(warmup):
            send_forward(forward_mb(recv_forward(fwd_idx), fwd_idx))
            fwd_idx += 1
        inp = recv_forward(fwd_idx) if steady > 0 else None
        for i in range(steady):
            out = forward_mb(inp, fwd_idx)
            fwd_idx += 1
            grad_out = send_fwd_recv_bwd(out)
            ingrad = backward_mb(grad_out, bwd_idx)
            bwd_idx += 1
            last_steady = i == steady - 1
            if not last_steady:
                if self.is_first:
                    inp = recv_forward(fwd_idx)
                elif ingrad is not None:
                    inp = send_bwd_recv_fwd(ingrad)
            else:
                send_backward(ingrad)
        for _ in range(warmup):  # cooldown: backward-only traffic, acyclic
            grad_out = (None if self.is_last
                        else self._recv_grad(fifo[0][1]))
            send_backward(backward_mb(grad_out, bwd_idx))
            bwd_idx += 1

        for w in send_works:
            w.wait()
        if step:
            with self.profiler.span(EventType.COMPUTE, "update_parameters"):
                self.optimizer.step()
                self.optimizer.zero_grad()
                if self.scheduler is not None:
                    self.scheduler.step()
        if losses:  # one host sync for the whole batch
            packed = torch.stack([torch.stack([l.detach() for l in losses]).sum(),
                                  torch.stack(accs).mean()])
            stats = {"loss": float(packed[0].detach()),
                     "accuracy": float(packed[1])}
        else:
            stats = {"loss": 0.0, "accuracy": 0.0}
        return stats

    @torch.no_grad()
    def eval_batch(self, x: Optional[torch.Tensor],
                   y: Optional[torch.Tensor]) -> Dict[str, float]:
        """Validation forward pass (reference async_val_batch)."""
        self.stage.eval()
        M = self.M
        if self.is_first:
            micro_x = list(x.to(self.device).chunk(M, dim=0))
            mb_size = micro_x[0].shape[0]
        else:
            mb_size = (x.shape[0] if x is not None else y.shape[0]) // M
        if self.is_last:
            micro_y = list(y.to(self.device).chunk(M, dim=0))
        loss_sum, acc_sum = 0.0, 0.0
        works = []
        for i in range(M):
            if self.is_first:
                inp = (micro_x[i].to(self.io_dtype)
                       if micro_x[i].is_floating_point() else micro_x[i])
            else:
                inp = torch.empty(mb_size, *self.in_shape, device=self.device,
                                  dtype=self.io_dtype)
                self.comm.recv(inp, self.rank - 1)
            out = self.stage(inp)
            if self.is_last:
                loss_sum += self.criterion(out, micro_y[i]).item() / M
                acc_sum += accuracy(out, micro_y[i]) / M
            else:
                works.append(self.comm.isend(out, self.rank + 1))
        for w in works:
            w.wait()
        return {"loss": loss_sum, "accuracy": acc_sum}

    def broadcast_stats(self, stats: Dict[str, float]) -> Dict[str, float]:
        return self.comm.broadcast_object(stats, src=self.world - 1)

    def state_dict(self):
        return self.stage.state_dict()

    # -- profiling control plane (reference coordinator.hpp:277-362:
    #    START/REPORT/CLEAR fan-out + merge) --------------------------------
    def start_profiling(self):
        self.profiler.start()

    def stop_profiling(self):
        self.profiler.stop()

    def gather_profiles(self) -> Optional[Profiler]:
        """Collect every rank's events on rank 0 (reference merges returned
        Profiler payloads, coordinator.hpp:291-362)."""
        dumps = self.comm.gather_objects(self.profiler.to_dict(), dst=0)
        if self.rank != 0:
            return None
        merged = Profiler("pipeline")
        for d in dumps:
            merged.merge(Profiler.from_dict(d))
        return merged

    def clear_profiling(self):
        self.profiler.clear()
