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

    ``open(batch)`` starts with empty rows instead of a prefill,
    ``extend(chunks)`` appends several tokens per row at each row's own
    position (a further turn, a refilled row, a prompt in pieces, draft
    tokens) and ``rewind(lengths)`` sets the positions back.
    ``verify(chunks)`` is ``extend`` for a block of draft tokens: the same
    forward on the split-KV extend kernel, returning the greedy token after
    every fed token (``generate_speculative``).
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

    def open(self, batch: int) -> None:
        """Live caches for ``batch`` rows, every row at length 0, without
        a prefill: fill them with ``extend``."""
        if batch < 1:
            raise ValueError("open wants at least one row")
        self.close()
        self.pos = torch.zeros(batch, dtype=torch.int64, device=self.device)
        for a in self._attns:
            a.enable_static_cache(self.seq_len, self.pos)
        for p in self._poss:
            p._pos_tensor = self.pos

    @torch.no_grad()
    def extend(self, chunks: List[List[int]],
               kv_splits: int = 0) -> torch.Tensor:
        """Append ``chunks[b]`` to row b at its own position: one eager
        forward over the right-padded ``[B, Tmax]`` batch, every row
        attending over its own cache prefix, the chunk lengths on the
        device. Returns the ``[B, V]`` logits at each row's last new token
        and advances the positions by the chunk lengths. A row with an
        empty chunk keeps its position, none of its live cache slots is
        written, and its logits are finite but mean nothing. Raises
        ``ValueError``, with nothing changed, if a row would pass
        ``seq_len`` (the positions are read back: one sync). Positions
        stay clamped to ``seq_len - 1`` like everywhere in this class, so
        a row filled to the brim reads as one short of it. ``kv_splits``
        goes to ``ops.attention_extend`` (0: the unsplit kernel)."""
        x, n_new = self._extend_input(chunks)
        logits = self._extend_logits(x, n_new, kv_splits)
        return logits[torch.arange(x.shape[0], device=self.device),
                      (n_new - 1).clamp(min=0)]

    def _extend_input(self, chunks: List[List[int]]):
        """Checked, right-padded ``[B, Tmax]`` tokens and device lengths."""
        if self.pos is None:
            raise RuntimeError("extend wants open() or prefill() first")
        B = self.pos.numel()
        lens = [len(c) for c in chunks]
        if len(chunks) != B:
            raise ValueError(f"extend wants {B} chunks, got {len(chunks)}")
        cur = self.pos.tolist()
        for b in range(B):
            if cur[b] + lens[b] > self.seq_len:
                raise ValueError(
                    f"extend: row {b} at {cur[b]} + {lens[b]} tokens passes "
                    f"seq_len {self.seq_len}")
        tmax = max(1, max(lens))
        x = torch.tensor([list(c) + [0] * (tmax - len(c)) for c in chunks],
                         dtype=torch.int64, device=self.device)
        n_new = torch.tensor(lens, dtype=torch.int64, device=self.device)
        return x, n_new

    def _extend_logits(self, x: torch.Tensor, n_new: torch.Tensor,
                       kv_splits) -> torch.Tensor:
        """The extend forward over ``x [B, Tmax]`` with ``n_new [B]`` live
        tokens per row: ``[B, Tmax, V]`` logits, positions advanced.
        ``kv_splits`` is a count, or a callable giving each attention
        block its own."""
        for a in self._attns:
            a.set_extend(True, n_new,
                         kv_splits(a) if callable(kv_splits) else kv_splits)
        for p in self._poss:
            p._extend = True
        try:
            logits = self.model(x)                   # [B, Tmax, V]
        finally:
            for a in self._attns:
                a.set_extend(False)
            for p in self._poss:
                p._extend = False
        self.pos.add_(n_new).clamp_(max=self.seq_len - 1)
        return logits

    def _verify_splits(self, tmax: int):
        """Per attention block, the split count of the automatic route:
        ``ext.attn_extend_splits`` where the bf16 extend kernel runs, 0
        elsewhere."""
        B = self.pos.numel()

        def splits(a) -> int:
            if not (self.device.type == "cuda"
                    and a.wq.dtype == torch.bfloat16
                    and a.head_dim in (64, 128)):
                return 0
            from .. import _C
            return _C.ext().attn_extend_splits(B * a.num_heads, self.seq_len,
                                               tmax)
        return splits

    @torch.no_grad()
    def verify(self, chunks: List[List[int]]) -> torch.Tensor:
        """The forward of ``extend`` for a block of draft tokens, on the
        split-KV extend kernel where the bf16 GPU route runs (split count
        from ``ext.attn_extend_splits``). Returns the greedy token after
        every fed token, int64 ``[B, Tmax]`` on the device
        (``ops.sample_logits`` at temperature 0: the lowest index among
        the maxima, as in the captured decode step); entries at and beyond
        a row's chunk length mean nothing. Positions advance as in
        ``extend``; the caller rewinds to what it accepts."""
        x, n_new = self._extend_input(chunks)
        return self._verify(x, n_new)

    def _verify(self, x: torch.Tensor, n_new: torch.Tensor) -> torch.Tensor:
        """``verify`` on device tensors, unchecked: the caller vouches that
        no row passes ``seq_len`` (no position read-back)."""
        from ..ops import sample_logits
        B, tmax = x.shape
        logits = self._extend_logits(x, n_new, self._verify_splits(tmax))
        return sample_logits(logits.reshape(B * tmax, -1),
                             temperature=0).reshape(B, tmax)

    def rewind(self, lengths: List[int]) -> None:
        """Set every row's position. Cache slots at and above a row's
        position are dead to every kernel, so this is all it takes to drop
        a turn or the tokens after an EOT."""
        if self.pos is None:
            raise RuntimeError("rewind wants open() or prefill() first")
        if len(lengths) != self.pos.numel() or any(
                not 0 <= n <= self.seq_len for n in lengths):
            raise ValueError("rewind wants one length in 0..seq_len per row")
        self.pos.copy_(torch.tensor(
            [min(n, self.seq_len - 1) for n in lengths], dtype=torch.int64))

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
def _decode_loop(dec: BatchedDecoder, logits: torch.Tensor, n_steps: int,
                 temp: float, top_k: int, top_p: float, seed: int,
                 is_greedy: bool, use_graph: Optional[bool]
                 ) -> List[List[int]]:
    """``n_steps`` tokens per row on an open decoder whose rows have just
    produced ``logits``: first pick, then the single-token step -- forward,
    on-device sampling, feed-back, id recording, position advance --
    captured once and replayed (or run eagerly), and one read-back of the
    ids ``[B][n_steps]``. Leaves every position advanced by ``n_steps -
    1``: the last token of a row is sampled but not fed."""
    from ..ops import sample_logits
    device = dec.device
    B = logits.shape[0]
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
    return ids_buf[:, :n_steps].tolist()


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
            n_steps = max(n_new[i] for i in rows)
            new = _decode_loop(dec, logits, n_steps, temp, top_k, top_p,
                               seed, is_greedy, use_graph)
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


def _vocab_and_positions(model: Sequential):
    """(vocabulary size, shortest positional table) of a GPT-style model."""
    from ..nn.layers import Embedding, PositionalEmbedding
    vocab = [m.vocab_size for m in model.modules() if isinstance(m, Embedding)]
    plen = [m.max_len for m in model.modules()
            if isinstance(m, PositionalEmbedding)]
    return (vocab[0] if vocab else None), (min(plen) if plen else None)


@torch.no_grad()
def _speculative_chunk(tgt: BatchedDecoder, drf: BatchedDecoder,
                       prompts: List[List[int]], n_new: List[int], k: int,
                       eot_token: Optional[int], use_graph: Optional[bool]):
    """Greedy draft/verify rounds for one batch of live rows (every
    ``n_new[b] >= 1``). Returns the new ids per row and (rounds, drafted,
    accepted). Invariant at the top of a round: both caches hold row b's
    first ``L_b`` tokens, both position tensors read ``L_b``, and the
    pending token (sampled, in neither cache) sits in ``pending``."""
    from ..ops import sample_logits
    device, seq_len = tgt.device, tgt.seq_len
    B = len(prompts)
    graphed = device.type == "cuda" if use_graph is None else use_graph

    logits = tgt.prefill(prompts)
    drf.prefill(prompts)
    pending = sample_logits(logits, temperature=0).reshape(B, 1)

    # the draft's single-token step, as _decode_loop captures its own:
    # forward, greedy pick, record, feed-back, advance
    step_t = torch.zeros(1, dtype=torch.int64, device=device)
    static_tok = pending.clone()
    # two spare columns: the graph warm-up steps record past the end
    d_buf = torch.zeros(B, k + 3, dtype=torch.int64, device=device)

    def step():
        nxt = sample_logits(drf.forward_token(static_tok),
                            temperature=0).reshape(B, 1)
        d_buf.index_copy_(1, step_t, nxt)
        static_tok.copy_(nxt)
        step_t.add_(1)
        drf.advance()

    graph = None
    if graphed:
        state = (drf.pos, static_tok, d_buf, step_t)
        saved = [t.clone() for t in state]
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            for _ in range(2):  # warmup; stale cache rows stay masked
                step()
        torch.cuda.current_stream().wait_stream(stream)
        for t, s0 in zip(state, saved):
            t.copy_(s0)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            step()
        for t, s0 in zip(state, saved):
            t.copy_(s0)

    first = pending[:, 0].tolist()
    new: List[List[int]] = [[t] for t in first]
    length = [len(p) for p in prompts]      # L_b, mirrored on the host
    done = [n_new[b] <= 1 or (eot_token is not None and first[b] == eot_token)
            for b in range(B)]
    rounds, drafted, accepted = 0, [0] * B, [0] * B
    col = torch.arange(k + 1, device=device)

    while not all(done):
        rounds += 1
        # 1. draft: k + 1 single-token steps from the pending token, the
        # last only to put d_k into the draft's cache
        static_tok.copy_(pending)
        step_t.zero_()
        for _ in range(k + 1):
            if graph is not None:
                graph.replay()
            else:
                step()
        # 2. verify [pending, d_1 .. d_k], cut to the slots a row has left
        lens = [0 if done[b] else min(k + 1, seq_len - length[b])
                for b in range(B)]
        tmax = max(lens)
        lens_t = torch.tensor(lens, dtype=torch.int64, device=device)
        # (a finished row may have been filled to the brim: keep it in bounds)
        old = torch.tensor([min(n, seq_len - 1) for n in length],
                           dtype=torch.int64, device=device)
        x = torch.cat([pending, d_buf[:, :k]], 1)[:, :tmax]
        # padding reads as token 0, as in extend
        x = torch.where(col[None, :tmax] < lens_t[:, None], x,
                        torch.zeros_like(x))
        tgt.pos.copy_(old)
        t_tok = tgt._verify(x, lens_t)                       # [B, tmax]
        # 3. accept: j leading drafts that the target would have picked
        ok = (x[:, 1:] == t_tok[:, :-1]) & \
            (col[None, 1:tmax] < lens_t[:, None])
        j = ok.long().cumprod(1).sum(1, keepdim=True)        # [B, 1]
        emit = torch.where(col[None, :tmax] < j,
                           torch.cat([x[:, 1:], x[:, :1]], 1), t_tok)
        pending = t_tok.gather(1, j)
        live_t = lens_t > 0
        new_pos = torch.where(live_t, old + j[:, 0] + 1, old) \
            .clamp_(max=seq_len - 1)
        tgt.pos.copy_(new_pos)
        drf.pos.copy_(new_pos)
        # 4. the round's one read-back
        back = torch.cat([emit, j], 1).tolist()
        for b in range(B):
            if done[b]:
                continue
            jb = back[b][tmax]
            ids = back[b][:jb + 1]
            drafted[b] += lens[b] - 1
            accepted[b] += jb
            length[b] += jb + 1
            room = n_new[b] - len(new[b])
            ids = ids[:room]
            if eot_token is not None and eot_token in ids:
                ids = ids[:ids.index(eot_token) + 1]
                done[b] = True
            new[b] += ids
            if len(new[b]) >= n_new[b]:
                done[b] = True
    return new, (rounds, drafted, accepted)


@torch.no_grad()
def generate_speculative(target: Sequential, draft: Sequential,
                         prompts: List[List[int]], max_new_tokens: int = 50,
                         k: int = 4, seq_len: int = 1024,
                         eot_token: Optional[int] = 50256,
                         device: Optional[torch.device] = None,
                         use_graph: Optional[bool] = None,
                         return_stats: bool = False):
    """Greedy speculative decode of a ragged batch: a small ``draft`` model
    proposes ``k`` tokens per row and round with its single-token step
    (captured once as a hipGraph and replayed), the ``target`` checks them
    in one ``BatchedDecoder.verify`` forward (split-KV extend attention on
    the bf16 GPU route) and each row keeps the drafts up to the first one
    the target would not have picked, plus the target's own token there:
    1 to ``k + 1`` tokens per target forward. Acceptance and the position
    updates stay on the device; the emitted tokens are read back once per
    round.

    Contract: for any draft, in fp32 the result equals
    ``generate_batch(target, prompts, greedy=True, ...)`` token for token,
    with its length rule (``min(max_new_tokens, seq_len - len)``, rows
    without room returned unchanged) and EOT truncation. More than 16
    prompts run in chunks of 16. ``1 <= k <= 15``. ``ValueError`` before
    any cache exists for differing vocabularies, a draft whose positional
    table is shorter than ``seq_len``, ``k`` out of range or an empty
    prompt. ``return_stats=True`` also returns ``{"rounds", "drafted",
    "accepted"}``, the last two per row. Greedy only: sampled speculative
    decoding (rejection sampling over both distributions) is not built."""
    prompts = [list(p) for p in prompts]
    if any(len(p) == 0 for p in prompts):
        raise ValueError("generate_speculative: empty prompt")
    if not 1 <= k <= 15:
        raise ValueError(f"k must be in 1..15, got {k}")
    (tv, _), (dv, dpos) = (_vocab_and_positions(m) for m in (target, draft))
    if tv != dv:
        raise ValueError(f"target and draft vocabularies differ: {tv} vs {dv}")
    if dpos is not None and dpos < seq_len:
        raise ValueError(f"the draft's positional table ({dpos}) is shorter "
                         f"than seq_len {seq_len}")
    device = device or next(target.parameters()).device
    n_new = [min(max_new_tokens, seq_len - len(p)) for p in prompts]
    out = [list(p) for p in prompts]
    live = [i for i, n in enumerate(n_new) if n > 0]
    stats = {"rounds": 0, "drafted": [0] * len(prompts),
             "accepted": [0] * len(prompts)}

    for c0 in range(0, len(live), MAX_DECODE_BATCH):
        rows = live[c0:c0 + MAX_DECODE_BATCH]
        tgt = BatchedDecoder(target, seq_len, device)
        drf = BatchedDecoder(draft, seq_len, device)
        try:
            new, (rounds, drafted, accepted) = _speculative_chunk(
                tgt, drf, [prompts[i] for i in rows],
                [n_new[i] for i in rows], k, eot_token, use_graph)
        finally:
            tgt.close()
            drf.close()
        stats["rounds"] += rounds
        for r, i in enumerate(rows):
            out[i] = prompts[i] + new[r]
            stats["drafted"][i] = drafted[r]
            stats["accepted"][i] = accepted[r]
    return (out, stats) if return_stats else out


class DecodeSession:
    """Multi-turn batched decode over live KV caches: up to 16 rows, each
    with its own growing context. ``generate(chunks)`` appends
    ``chunks[b]`` to row b's context with one ``extend`` forward (no
    re-prefill of what was said before), decodes all rows together with
    the captured single-token step of ``generate_batch`` and returns the
    new tokens per row, EOT-truncated.

    A row with an empty chunk is idle in that call: it returns ``[]``, its
    context and live cache are unchanged, and its position is restored
    after the shared steps (which write only dead slots above it). An
    active row yields ``min(max_new_tokens, seq_len - len(context) -
    len(chunk))`` tokens. The last sampled token of a row is not in the
    cache yet: the session keeps ``pos_b = len(context_b) - 1`` and feeds
    that pending token in front of the next chunk. Rewinding to that
    position also drops whatever the shared steps wrote past a row's EOT.

    Greedy contract: row b's result equals the new tokens of
    ``generate_batch(model, [context_b + chunk_b], ...)`` with the same
    ``max_new_tokens``, ``seq_len`` and ``eot_token``.

    ``context`` is the host copy of every row's tokens; ``rewind(lengths)``
    cuts contexts back; ``reset(rows)`` frees rows (all when None) by
    setting their length to 0; ``close()`` drops the caches."""

    def __init__(self, model: Sequential, batch: int, seq_len: int = 1024,
                 device: Optional[torch.device] = None):
        if not 1 <= batch <= MAX_DECODE_BATCH:
            raise ValueError(
                f"DecodeSession wants 1..{MAX_DECODE_BATCH} rows, got {batch}")
        self.seq_len = seq_len
        self.context: List[List[int]] = [[] for _ in range(batch)]
        self._dec = BatchedDecoder(model, seq_len, device)
        self._dec.open(batch)

    def _sync_positions(self) -> None:
        self._dec.rewind([max(len(c) - 1, 0) for c in self.context])

    @torch.no_grad()
    def generate(self, chunks: List[List[int]], max_new_tokens: int = 50,
                 eot_token: Optional[int] = 50256, greedy: bool = True,
                 temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0,
                 seed: int = 0, use_graph: Optional[bool] = None
                 ) -> List[List[int]]:
        if self._dec.pos is None:
            raise RuntimeError("DecodeSession is closed")
        chunks = [list(c) for c in chunks]
        B = len(self.context)
        if len(chunks) != B:
            raise ValueError(f"generate wants {B} chunks, got {len(chunks)}")
        if not (0.0 < top_p <= 1.0):
            raise ValueError(f"top_p must be in (0, 1], got {top_p}")
        if top_k < 0:
            raise ValueError(f"top_k must be >= 0, got {top_k}")
        if temperature < 0:
            raise ValueError(f"temperature must be >= 0, got {temperature}")
        for b in range(B):
            if len(self.context[b]) + len(chunks[b]) > self.seq_len:
                raise ValueError(
                    f"generate: row {b} would pass seq_len {self.seq_len}")
        temp = 0.0 if greedy else float(temperature)
        is_greedy = temp == 0.0 or top_k == 1
        n_new = [min(max_new_tokens, self.seq_len - len(self.context[b])
                     - len(chunks[b])) if chunks[b] else 0 for b in range(B)]
        out: List[List[int]] = [[] for _ in range(B)]
        if not any(chunks):
            return out
        # the pending (sampled, not yet cached) token leads the chunk
        feeds = [self.context[b][-1:] + chunks[b] if chunks[b] else []
                 for b in range(B)]
        try:
            logits = self._dec.extend(feeds)
            n_steps = max(n_new)
            if n_steps > 0:
                new = _decode_loop(self._dec, logits, n_steps, temp, top_k,
                                   top_p, seed, is_greedy, use_graph)
                for b in range(B):
                    ids = new[b][:max(n_new[b], 0)]
                    if eot_token is not None and eot_token in ids:
                        ids = ids[:ids.index(eot_token) + 1]
                    out[b] = ids
            for b in range(B):
                self.context[b] += chunks[b] + out[b]
        finally:
            self._sync_positions()
        return out

    def rewind(self, lengths: List[int]) -> None:
        """Cut row b's context back to its first ``lengths[b]`` tokens
        (drops a turn; the cache slots behind them go dead)."""
        if len(lengths) != len(self.context) or any(
                not 0 <= n <= len(c) for n, c in zip(lengths, self.context)):
            raise ValueError("rewind wants one length within each context")
        self.context = [c[:n] for c, n in zip(self.context, lengths)]
        self._sync_positions()

    def reset(self, rows: Optional[List[int]] = None) -> None:
        for b in (range(len(self.context)) if rows is None else rows):
            self.context[b] = []
        self._sync_positions()

    def close(self) -> None:
        self._dec.close()
