"""Autoregressive generation (reference examples/gpt2_inference.cpp:19-127).

The reference recomputes the full sequence per token (:71-122, explicitly
no KV cache). ``generate`` reproduces that; ``generate_cached`` adds the
KV-cache fast path the reference lacks, exploiting that every layer in the
GPT zoo is causal: past activations are position-invariant, so we only
recompute the suffix window when the prompt overflows.
"""

from __future__ import annotations

from typing import List, Optional

import torch

from ..nn.blocks import Sequential


@torch.no_grad()
def generate(model: Sequential, prompt_ids: List[int], max_new_tokens: int = 50,
             seq_len: int = 1024, eot_token: Optional[int] = 50256,
             device: Optional[torch.device] = None,
             greedy: bool = True, temperature: float = 1.0) -> List[int]:
    """Greedy/sampled decode with full-sequence recompute per token."""
    device = device or next(model.parameters()).device
    model.eval()
    ids = list(prompt_ids)
    for _ in range(max_new_tokens):
        window = ids[-seq_len:]
        x = torch.tensor([window], dtype=torch.int64, device=device)
        logits = model(x)[0, len(window) - 1]
        if greedy:
            nxt = int(logits.argmax().item())
        else:
            probs = torch.softmax(logits.float() / temperature, dim=-1)
            nxt = int(torch.multinomial(probs, 1).item())
        ids.append(nxt)
        if eot_token is not None and nxt == eot_token:
            break
    return ids


@torch.no_grad()
def generate_cached(model: Sequential, prompt_ids: List[int],
                    max_new_tokens: int = 50, seq_len: int = 1024,
                    eot_token: Optional[int] = 50256,
                    device: Optional[torch.device] = None,
                    greedy: bool = True, temperature: float = 1.0) -> List[int]:
    """KV-cached decode: prefill once, then one token per step."""
    from ..nn.blocks import _MHABase
    from ..nn.layers import PositionalEmbedding
    device = device or next(model.parameters()).device
    model.eval()
    attns = [m for m in model.modules() if isinstance(m, _MHABase)]
    poss = [m for m in model.modules() if isinstance(m, PositionalEmbedding)]
    for a in attns:
        a.enable_cache(max_len=seq_len)
    try:
        ids = list(prompt_ids)
        x = torch.tensor([ids], dtype=torch.int64, device=device)
        logits = model(x)[0, -1]
        for t in range(max_new_tokens):
            if greedy:
                nxt = int(logits.argmax().item())
            else:
                probs = torch.softmax(logits.float() / temperature, dim=-1)
                nxt = int(torch.multinomial(probs, 1).item())
            ids.append(nxt)
            if eot_token is not None and nxt == eot_token:
                break
            if len(ids) >= seq_len:
                break
            for p in poss:
                p._pos_offset = len(ids) - 1
            step = torch.tensor([[nxt]], dtype=torch.int64, device=device)
            logits = model(step)[0, -1]
        return ids
    finally:
        for a in attns:
            a.reset_cache()
        for p in poss:
            p._pos_offset = 0


@torch.no_grad()
def generate_graphed(model: Sequential, prompt_ids: List[int],
                     max_new_tokens: int = 50, seq_len: int = 1024,
                     eot_token: Optional[int] = 50256,
                     device: Optional[torch.device] = None,
                     use_graph: Optional[bool] = None) -> List[int]:
    """hipGraph-captured, fully GPU-resident greedy decode.

    The per-token step -- forward over fixed-capacity KV buffers, argmax,
    feeding the result back into the static input, recording it into a
    device id buffer, and advancing the device position counter -- is
    captured once and replayed per token with ZERO host round-trips;
    the generated ids are read back in one transfer at the end. EOT
    handling is post-hoc truncation (identical output to ``generate``).
    ``use_graph=False`` runs the identical tensor-driven step eagerly
    (CPU-testable path)."""
    from ..nn.blocks import _MHABase
    from ..nn.layers import PositionalEmbedding
    device = device or next(model.parameters()).device
    if use_graph is None:
        use_graph = device.type == "cuda"
    model.eval()
    attns = [m for m in model.modules() if isinstance(m, _MHABase)]
    poss = [m for m in model.modules() if isinstance(m, PositionalEmbedding)]
    pos_t = torch.zeros(1, dtype=torch.int64, device=device)
    for a in attns:
        a.enable_static_cache(seq_len, pos_t)
    try:
        ids = list(prompt_ids)
        plen = len(ids)
        total_new = min(max_new_tokens, seq_len - plen)
        if total_new <= 0:
            return ids
        x = torch.tensor([ids], dtype=torch.int64, device=device)
        logits = model(x)[0, -1]           # prefill (eager, fills caches)
        first = logits.argmax().reshape(1, 1)
        pos_t.fill_(plen)
        for p in poss:
            p._pos_tensor = pos_t
        static_tok = first.clone()
        ids_buf = torch.zeros(seq_len, dtype=torch.int64, device=device)
        ids_buf[plen] = first[0, 0]

        def step():
            out = model(static_tok)[:, -1]          # [1, V]
            nxt = out.argmax(-1, keepdim=True)      # [1, 1]
            pos_t.add_(1)
            ids_buf.index_copy_(0, pos_t, nxt[0])
            static_tok.copy_(nxt)

        n_replay = total_new - 1
        if use_graph and n_replay > 0:
            saved = (pos_t.clone(), static_tok.clone(), ids_buf.clone())
            stream = torch.cuda.Stream()
            stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(stream):
                for _ in range(2):      # warmup; stale cache rows stay masked
                    step()
            torch.cuda.current_stream().wait_stream(stream)
            pos_t.copy_(saved[0]); static_tok.copy_(saved[1])
            ids_buf.copy_(saved[2])
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                step()
            pos_t.copy_(saved[0]); static_tok.copy_(saved[1])
            ids_buf.copy_(saved[2])
            for _ in range(n_replay):
                graph.replay()
        else:
            for _ in range(n_replay):
                step()
        new_ids = ids_buf[plen:plen + total_new].tolist()
        if eot_token is not None and eot_token in new_ids:
            new_ids = new_ids[:new_ids.index(eot_token) + 1]
        return ids + new_ids
    finally:
        for a in attns:
            a.reset_cache()
        for p in poss:
            p._pos_tensor = None


class BatchedDecoder:
    """Static-cache decoder over a ragged batch: one device position per
    sequence, so every single-token step is one fixed-shape forward over
    all B rows (hipGraph-capturable, no host round-trips).

    ``prefill(prompts)`` runs one eager forward over the right-padded
    ``[B, Lmax]`` batch and returns row b's logits at ``len_b - 1``. That
    is exact: every layer is causal, so real tokens never attend to the
    padding behind them, and the padding's K/V rows at ``>= len_b`` are
    overwritten or masked because decode starts at ``pos_b = len_b``.
    ``step(tokens)`` feeds one caller-chosen token per row at its
    position, returns the next-token logits ``[B, V]`` and advances the
    positions, clamped to ``seq_len - 1`` so a full row stays in bounds
    (its further outputs are meaningless). ``close()`` drops the caches.
    """

    def __init__(self, model: Sequential, seq_len: int = 1024,
                 device: Optional[torch.device] = None):
        from ..nn.blocks import _MHABase
        from ..nn.layers import PositionalEmbedding
        self.model, self.seq_len = model, seq_len
        self.device = device or next(model.parameters()).device
        model.eval()
        self._attns = [m for m in model.modules() if isinstance(m, _MHABase)]
        self._poss = [m for m in model.modules()
                      if isinstance(m, PositionalEmbedding)]
        self.pos: Optional[torch.Tensor] = None

    @torch.no_grad()
    def prefill(self, prompts: List[List[int]]) -> torch.Tensor:
        lens = [len(p) for p in prompts]
        if not prompts or min(lens) < 1 or max(lens) > self.seq_len:
            raise ValueError("prefill wants prompts of 1..seq_len tokens")
        self.close()
        B, lmax = len(prompts), max(lens)
        self.pos = torch.zeros(B, dtype=torch.int64, device=self.device)
        for a in self._attns:
            a.enable_static_cache(self.seq_len, self.pos)
        x = torch.tensor([list(p) + [0] * (lmax - len(p)) for p in prompts],
                         dtype=torch.int64, device=self.device)
        lens_t = torch.tensor(lens, dtype=torch.int64, device=self.device)
        logits = self.model(x)                       # [B, Lmax, V]
        out = logits[torch.arange(B, device=self.device), lens_t - 1]
        self.pos.copy_(lens_t.clamp(max=self.seq_len - 1))
        for p in self._poss:
            p._pos_tensor = self.pos
        return out

    def forward_token(self, tok: torch.Tensor) -> torch.Tensor:
        """Logits ``[B, V]`` for the ``[B, 1]`` tokens at the current
        positions; does not advance."""
        return self.model(tok)[:, -1]

    def advance(self) -> None:
        self.pos.add_(1).clamp_(max=self.seq_len - 1)

    @torch.no_grad()
    def step(self, tokens) -> torch.Tensor:
        tok = torch.as_tensor(tokens, dtype=torch.int64,
                              device=self.device).reshape(-1, 1)
        logits = self.forward_token(tok)
        self.advance()
        return logits

    def close(self) -> None:
        for a in self._attns:
            a.reset_cache()
        for p in self._poss:
            p._pos_tensor = None
        self.pos = None


MAX_DECODE_BATCH = 16   # rows of one captured step (the skinny GEMM's M)


@torch.no_grad()
def generate_batch(model: Sequential, prompts: List[List[int]],
                   max_new_tokens: int = 50, seq_len: int = 1024,
                   eot_token: Optional[int] = 50256,
                   device: Optional[torch.device] = None,
                   greedy: bool = True, temperature: float = 1.0,
                   top_k: int = 0, top_p: float = 1.0, seed: int = 0,
                   use_graph: Optional[bool] = None) -> List[List[int]]:
    """Decode a ragged batch of prompts together, GPU-resident.

    One padded prefill, then a single-token step over all rows -- forward,
    on-device sampling (``ops.sample_logits``: greedy, or temperature /
    top-k / top-p), feed-back, id recording and position advance --
    captured once as a hipGraph and replayed with no host round-trips;
    the ids are read back once at the end. The weights are streamed once
    per step for the whole batch. Row b yields ``min(max_new_tokens,
    seq_len - len_b)`` tokens (rows with none are returned unchanged);
    EOT is post-hoc truncation per row, as in ``generate_graphed``. More
    than 16 prompts run in chunks of 16. ``use_graph=False`` runs the
    identical tensor-driven step eagerly (CPU-testable path)."""
    from ..ops import sample_logits
    prompts = [list(p) for p in prompts]
    if any(len(p) == 0 for p in prompts):
        raise ValueError("generate_batch: empty prompt")
    if not (0.0 < top_p <= 1.0):
        raise ValueError(f"top_p must be in (0, 1], got {top_p}")
    if top_k < 0:
        raise ValueError(f"top_k must be >= 0, got {top_k}")
    if temperature < 0:
        raise ValueError(f"temperature must be >= 0, got {temperature}")
    device = device or next(model.parameters()).device
    temp = 0.0 if greedy else float(temperature)
    is_greedy = temp == 0.0 or top_k == 1
    n_new = [min(max_new_tokens, seq_len - len(p)) for p in prompts]
    out = [list(p) for p in prompts]
    live = [i for i, n in enumerate(n_new) if n > 0]

    def run_chunk(rows: List[int]) -> None:
        dec = BatchedDecoder(model, seq_len, device)
        try:
            logits = dec.prefill([prompts[i] for i in rows])
            B = len(rows)
            n_steps = max(n_new[i] for i in rows)
            graph_ok = device.type == "cuda" and (
                is_greedy or logits.dtype == torch.bfloat16)
            graphed = graph_ok if use_graph is None else use_graph
            step_t = torch.zeros(1, dtype=torch.int64, device=device)

            def pick(lg):
                return sample_logits(lg, temp, top_k, top_p, seed, step_t)

            # two spare columns: the graph warm-up steps record past the end
            ids_buf = torch.zeros(B, n_steps + 2, dtype=torch.int64,
                                  device=device)
            first = pick(logits)
            ids_buf[:, 0] = first
            static_tok = first.reshape(B, 1).clone()
            step_t.fill_(1)

            def step():
                nxt = pick(dec.forward_token(static_tok)).reshape(B, 1)
                ids_buf.index_copy_(1, step_t, nxt)
                static_tok.copy_(nxt)
                step_t.add_(1)
                dec.advance()

            state = (dec.pos, static_tok, ids_buf, step_t)
            n_replay = n_steps - 1
            if graphed and n_replay > 0:
                saved = [t.clone() for t in state]

                def restore():
                    for t, s0 in zip(state, saved):
                        t.copy_(s0)

                stream = torch.cuda.Stream()
                stream.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(stream):
                    for _ in range(2):  # warmup; stale cache rows stay masked
                        step()
                torch.cuda.current_stream().wait_stream(stream)
                restore()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    step()
                restore()
                for _ in range(n_replay):
                    graph.replay()
            else:
                for _ in range(n_replay):
                    step()
            new = ids_buf[:, :n_steps].tolist()
            for r, i in enumerate(rows):
                ids = new[r][:n_new[i]]
                if eot_token is not None and eot_token in ids:
                    ids = ids[:ids.index(eot_token) + 1]
                out[i] = prompts[i] + ids
        finally:
            dec.close()

    for c0 in range(0, len(live), MAX_DECODE_BATCH):
        run_chunk(live[c0:c0 + MAX_DECODE_BATCH])
    return out
