"""Host side of the flow-matching decoder: mirrors `CausalMaskedDiffWithDiT.inference`
(CosyVoice/cosyvoice/flow/flow.py:358-403) and the estimator hand-off of
`ConditionalCFM.forward_estimator` (flow/flow_matching.py:126-153) over the C ABI."""
from __future__ import annotations

import ctypes as C
from collections import deque
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import FY_DIRECT, FY_NO_FINALIZE, FY_PRECISE, FY_STREAMING, check  # noqa: F401
from .spec import FlowCfg


def reference_t_span(n_timesteps: int) -> torch.Tensor:
    """flow_matching.py:223-225, the same torch ops so the fp32 values are the reference's."""
    t = torch.linspace(0, 1, n_timesteps + 1, dtype=torch.float32)
    return 1 - torch.cos(t * 0.5 * torch.pi)


def stream_chunk_plan(n_tokens: int, n_prompt_tokens: int, hop: int = 25, look: int = 3):
    """The reference's stream=True chunk schedule (cli/model.py:339-369) as a pure function of the token count: a chunk is cut
    whenever hop + look tokens beyond the offset exist, the first hop padded so that prompt + hop is a multiple of `hop`; the
    rest is the final pass.  -> [(n_in, offset, finalize)]: the call sees tokens [:n_in] and yields the mel of tokens
    [offset : n_in - look] (finalize: [offset : n_in])."""
    pad = -(-n_prompt_tokens // hop) * hop - n_prompt_tokens
    plan, offset = [], 0
    while True:
        need = offset + (hop + pad if offset == 0 else hop) + look
        if need > n_tokens:
            break
        plan.append((need, offset, False))
        offset = need - look
    plan.append((n_tokens, offset, True))
    return plan


def stream_poll_plan(n_tokens: Sequence[int], n_prompt_tokens: Sequence[int], tokens_per_poll: int = 25, hop: int = 25, look: int = 3):
    """The schedule of K streams that share one lane (CosyVoice3Model.tts_stream_batch): every poll the LM adds up to
    `tokens_per_poll` tokens to each unfinished stream, then ONE batched flow call takes every stream whose next chunk is complete
    (at most one chunk per stream and poll) and one batched final pass the streams whose tokens have ended.
    -> [poll] of [(stream, n_in, offset, finalize)]; a stream's own entries are `stream_chunk_plan`'s, whoever else is live."""
    K = len(n_tokens)
    have, offset, ended = [0] * K, [0] * K, [False] * K
    pads = [-(-p // hop) * hop - p for p in n_prompt_tokens]
    polls = []
    while not all(ended):
        poll = []
        for i in range(K):
            if ended[i]:
                continue
            have[i] = min(n_tokens[i], have[i] + tokens_per_poll)
            need = offset[i] + (hop + pads[i] if offset[i] == 0 else hop) + look
            if have[i] >= need:
                poll.append((i, need, offset[i], False))
                offset[i] = need - look
            elif have[i] == n_tokens[i]:
                poll.append((i, n_tokens[i], offset[i], True))
                ended[i] = True
        polls.append(poll)
    return polls


class ServeStreamSchedule:
    """Every decision of the streaming serving loop (`CosyVoice3Model.tts_serve_stream`), as host state without a GPU: which
    request joins which slot, which chunk each stream gets in a poll and which slots fall free.  `plan_serve_stream` drives it
    with forced lengths, the loop with what the device reports; neither decides anything else.  One poll is: `arrive` for the
    requests that came in, `join`, the token steps (the caller's), `chunks` with the slots' counts, `next_poll`.
    A stream is credited at most `tokens_per_poll` tokens per poll, the join's own first token included (the device, which steps
    every slot `tokens_per_poll` times after the join, is one token ahead until it ends): the schedule of a stream is then
    `stream_poll_plan`'s from the poll it joins in, a function of its final count alone."""

    def __init__(self, n_slots: int, tokens_per_poll: int = 25, hop: int = 25, look: int = 3):
        assert n_slots >= 1 and tokens_per_poll >= 1 and hop >= 1 and look >= 0
        self.n_slots, self.tokens_per_poll, self.hop, self.look = int(n_slots), int(tokens_per_poll), int(hop), int(look)
        self.pending: deque = deque()             # (request, prompt tokens) that arrived and hold no slot yet, in arrival order
        self.occupied: Dict[int, int] = {}        # slot -> request
        self._have: Dict[int, int] = {}           # slot -> tokens credited
        self._offset: Dict[int, int] = {}         # slot -> tokens whose mel has been cut
        self._pad: Dict[int, int] = {}
        self._freed: List[int] = []               # released in this poll: free from the next one
        self.poll = 0

    def arrive(self, request: int, n_prompt_tokens: int):
        self.pending.append((request, int(n_prompt_tokens)))

    def join(self) -> List[Tuple[int, int]]:
        """The poll's one join: waiting requests in arrival order into the lowest free slots -> [(request, slot)]."""
        free = [s for s in range(self.n_slots) if s not in self.occupied and s not in self._freed]
        batch = []
        for s in free[: len(self.pending)]:
            r, p = self.pending.popleft()
            self.occupied[s] = r
            self._have[s], self._offset[s], self._pad[s] = 0, 0, -(-p // self.hop) * self.hop - p
            batch.append((r, s))
        return batch

    def need(self, slot: int) -> int:
        """Tokens the slot's next streaming chunk takes in."""
        o = self._offset[slot]
        return o + (self.hop + self._pad[slot] if o == 0 else self.hop) + self.look

    def chunks(self, counts: Dict[int, Tuple[int, bool]]):
        """counts: {occupied slot: (tokens its LM has emitted, whether it has ended)}.  In ascending slot order, at most one entry
        per stream: a streaming chunk when the credited tokens reach `need`, else the final pass when the LM has ended and every
        token is credited; that slot is released.  -> ([(request, n_in, offset, finalize)], [slot of each entry], released)."""
        out, slots, released = [], [], []
        for s in sorted(self.occupied):
            n, ended = counts[s]
            self._have[s] = min(int(n), self._have[s] + self.tokens_per_poll)
            need = self.need(s)
            if self._have[s] >= need:
                out.append((self.occupied[s], need, self._offset[s], False))
                slots.append(s)
                self._offset[s] = need - self.look
            elif ended and self._have[s] == int(n):
                out.append((self.occupied[s], int(n), self._offset[s], True))
                slots.append(s)
                released.append(s)
        for s in released:
            self.release(s)
        return out, slots, released

    def release(self, slot: int):
        """The slot's stream is over (its final pass, or no token at all): free from the next poll on."""
        del self.occupied[slot], self._have[slot], self._offset[slot], self._pad[slot]
        self._freed.append(slot)

    def next_poll(self):
        self._freed = []
        self.poll += 1

    @property
    def idle(self) -> bool:
        return not (self.pending or self.occupied)


def plan_serve_stream(n_tokens: Sequence[int], n_prompt_tokens: Sequence[int], arrivals: Optional[Sequence[int]], n_slots: int,
                      tokens_per_poll: int = 25, hop: int = 25, look: int = 3):
    """The schedule `CosyVoice3Model.tts_serve_stream` runs when request r arrives in poll arrivals[r] (non-decreasing; None: all
    in poll 0) with n_prompt_tokens[r] flow prompt tokens and its LM emits exactly n_tokens[r] tokens.  A pure function, no GPU.
    Poll p: the requests with arrivals[r] <= p wait in arrival order; ONE join puts them into the lowest free slots (the join emits
    the first token); every occupied slot's LM gains tokens, `tokens_per_poll` per poll counted from the join; every stream then
    gets at most one chunk - its next `stream_chunk_plan` entry once its tokens are there, the final pass in the poll that sees it
    ended; a slot released in a poll can be joined in the next.
    -> one dict per poll: {"joins": [(request, slot)], "chunks": [(request, n_in, offset, finalize)], "released": [slot]}; chunks in
    ascending slot order.  With every request present at poll 0 and no more requests than slots the chunk lists are
    `stream_poll_plan`'s."""
    N = len(n_tokens)
    arrivals = [0] * N if arrivals is None else [int(a) for a in arrivals]
    assert len(arrivals) == N and len(n_prompt_tokens) == N and all(int(n) >= 1 for n in n_tokens)
    assert all(a >= 0 for a in arrivals) and all(arrivals[i] <= arrivals[i + 1] for i in range(N - 1)), "arrival polls in request order"
    sch = ServeStreamSchedule(n_slots, tokens_per_poll, hop, look)
    nxt, polls = 0, []
    while nxt < N or not sch.idle:
        while nxt < N and arrivals[nxt] <= sch.poll:
            sch.arrive(nxt, n_prompt_tokens[nxt])
            nxt += 1
        joins = sch.join()
        chunks, _, released = sch.chunks({s: (int(n_tokens[r]), True) for s, r in sch.occupied.items()})
        polls.append({"joins": joins, "chunks": chunks, "released": released})
        sch.next_poll()
    return polls


def packed_rows(T: Sequence[int]):
    """The layout of a packed call (FY_PACKED, include/fy_cosy3.h) as a pure function of the utterances' mel rows T[b] (prompt +
    generated frames): the 2 B sequences - 2 b the conditional one of utterance b, 2 b + 1 its CFG branch - lie back to back in
    that order, T[b] rows each, frame after frame.  -> (offsets, Mp): sequence 2 b + s starts at compact row offsets[2 b + s],
    and Mp = 2 sum(T) rows go through the DiT blocks."""
    offsets, Mp = [], 0
    for b, t in enumerate(T):
        t = int(t)
        if t < 1:
            raise ValueError(f"utterance {b} has no rows (T = {t})")
        offsets += [Mp, Mp + t]
        Mp += 2 * t
    return offsets, Mp


def _cfg_struct(cfg: FlowCfg) -> _lib.FlowConfig:
    c = _lib.FlowConfig()
    _lib.lib().fy_flow_default_config(C.byref(c))
    c.mel, c.spk_in, c.vocab, c.pre_ch, c.pre_lookahead = cfg.mel, cfg.spk_in, cfg.vocab, cfg.pre_ch, cfg.pre_lookahead
    c.dim, c.depth, c.heads, c.head_dim, c.ff_mult = cfg.dim, cfg.depth, cfg.heads, cfg.head_dim, cfg.ff_mult
    c.conv_pos_k, c.conv_pos_groups, c.n_timesteps = cfg.conv_pos_k, cfg.conv_pos_groups, cfg.n_timesteps
    c.cfg_rate, c.static_chunk = cfg.cfg_rate, cfg.static_chunk
    for i, v in enumerate(reference_t_span(cfg.n_timesteps).tolist()):
        c.t_span[i] = v
    return c


class FlowEngine:
    """weights: the flow.pt state_dict (reference key names, fp32 CUDA tensors)."""

    token_mel_ratio = 2
    pre_lookahead_len = 3

    def __init__(self, weights: Dict[str, torch.Tensor], cfg: FlowCfg = FlowCfg(), max_batch: int = 8,
                 max_frames: int = 1500, device: Optional[torch.device] = None):
        self.cfg = cfg
        self.device = device or next(iter(weights.values())).device
        self.max_batch, self.max_frames = max_batch, max_frames
        self._h = C.c_void_p()
        arr, keep = _lib.tensor_table(weights)
        cs = _cfg_struct(cfg)
        with torch.cuda.device(self.device):
            check(_lib.lib().fy_flow_create(C.byref(self._h), C.byref(cs), arr, len(weights), max_batch, max_frames, self._stream()))
        del keep

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def close(self):
        if self._h:
            _lib.lib().fy_flow_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def inference(self, token: torch.Tensor, n_token: Sequence[int], prompt_token: torch.Tensor, n_prompt: Sequence[int],
                  prompt_feat: torch.Tensor, n_pfeat: Sequence[int], embedding: torch.Tensor, rand_noise: torch.Tensor,
                  flags: int = 0, streaming: bool = False, finalize: bool = True, incremental: bool = False,
                  packed: bool = False) -> torch.Tensor:
        """token (B, Nmax) int32, prompt_token (B, Pmax) int32, prompt_feat (B, PMmax, 80), embedding (B, 192),
        rand_noise (1|-, 80, >=T) -> mel (B, 80, 2*max(n_token)); utterance b is valid in [:, :, :2*n_token[b]].
        streaming / finalize as in the reference (flow.py:358-403): the chunk attention mask, and the last
        pre_lookahead tokens as look-ahead context only (valid frames 2*(n_token[b] - pre_lookahead)).
        incremental (with streaming, finalize=False, one utterance): this call extends the previous incremental call of the handle -
        only the new rows go through the DiT blocks (FY_INCREMENTAL; `stream_reset` starts a new stream).  Same result.  Works in
        the default arithmetic and with flags=FY_PRECISE (a call in the other arithmetic than the kept rows' starts over); with
        FY_DIRECT the call is computed whole.
        packed: a ragged batch sends only its valid rows through the DiT blocks (FY_PACKED; `packed_rows` is the layout,
        `last_rows` tells what ran).  Same result, bit for bit; with one utterance or equal lengths it is the padded call."""
        if packed:
            flags |= _lib.FY_PACKED
        if incremental:
            flags |= _lib.FY_INCREMENTAL
        if streaming:
            flags |= FY_STREAMING
        if not finalize:
            flags |= FY_NO_FINALIZE
        B = token.shape[0]
        dev = self.device
        token = token.to(dev, torch.int32).contiguous()
        prompt_token = prompt_token.to(dev, torch.int32).contiguous()
        if prompt_token.shape[1] == 0:
            prompt_token = torch.zeros(B, 1, dtype=torch.int32, device=dev)
        prompt_feat = prompt_feat.to(dev, torch.float32).contiguous()
        if prompt_feat.shape[1] == 0:
            prompt_feat = torch.zeros(B, 1, self.cfg.mel, device=dev)
        embedding = embedding.to(dev, torch.float32).contiguous()
        noise = rand_noise.reshape(self.cfg.mel, -1).to(dev, torch.float32).contiguous()
        frames = 2 * max(int(n) for n in n_token)
        mel = torch.zeros(B, self.cfg.mel, frames, device=dev, dtype=torch.float32)
        check(_lib.lib().fy_flow_infer(self._h, token.data_ptr(), token.shape[1], _lib.int_array(n_token),
                                       prompt_token.data_ptr(), prompt_token.shape[1], _lib.int_array(n_prompt),
                                       prompt_feat.data_ptr(), prompt_feat.shape[1], _lib.int_array(n_pfeat),
                                       embedding.data_ptr(), noise.data_ptr(), noise.shape[1], B, mel.data_ptr(), frames,
                                       flags, self._stream()))
        return mel

    @property
    def weight_planes(self) -> int:
        """1: the weights were bf16-representable; 2: a general fp32 checkpoint (lo planes kept for FY_PRECISE)."""
        return int(_lib.lib().fy_flow_weight_planes(self._h))

    @property
    def last_rows(self) -> int:
        """Rows the last `inference` call pushed through each DiT block's products: 2 B Tmax padded, 2 sum(T) packed,
        2 (T - T0) for an incremental call; 0 before any call."""
        return int(_lib.lib().fy_flow_last_rows(self._h))

    @property
    def ln_fold(self) -> bool:
        """Whether the handle built the folded LayerNorm-modulate tables at create (fy_flow_ln_fold)."""
        return int(_lib.lib().fy_flow_ln_fold(self._h)) == 1

    def stream_reset(self):
        """Forget what incremental calls have kept: the next one starts a new stream."""
        check(_lib.lib().fy_flow_stream_reset(self._h))

    def stream_rows(self) -> int:
        """Mel rows the incremental calls of the current stream have kept (0: the next call computes everything)."""
        return int(_lib.lib().fy_flow_stream_rows(self._h))

    # ---- stream slots: several stream=True utterances share one chunk pass (include/fy_cosy3.h) ----
    def open_streams(self, n_slots: int, cap_frames: int, precise: bool = False):
        """A session of n_slots incremental caches of cap_frames mel rows (prompt + generated) each; raises FyError when the
        device does not have the memory (2.7 MB per frame row and slot at full size).  precise: the session also takes
        `inference_streams(..., flags=FY_PRECISE)` (its first such call allocates the lo planes, the same bytes again); a session
        opened without it refuses that flag, as it always has."""
        with torch.cuda.device(self.device):
            check(_lib.lib().fy_flow_streams_open(self._h, n_slots, cap_frames))
            if precise:
                check(_lib.lib().fy_flow_streams_precise(self._h, 1))

    def close_streams(self):
        check(_lib.lib().fy_flow_streams_close(self._h))

    @property
    def streams_bytes(self) -> int:
        """Device bytes of the open stream-slot session (0: none); the lo planes of FY_PRECISE count from the first precise call."""
        return int(_lib.lib().fy_flow_streams_bytes(self._h))

    def stream_slot_reset(self, slot: int):
        """The slot's next `inference_streams` call starts a new stream."""
        check(_lib.lib().fy_flow_stream_slot_reset(self._h, slot))

    def stream_slot_rows(self, slot: int) -> int:
        """Mel rows the slot's stream has kept (0: its next call computes everything)."""
        return int(_lib.lib().fy_flow_stream_slot_rows(self._h, slot))

    def inference_streams(self, slots: Sequence[int], token: torch.Tensor, n_token: Sequence[int], prompt_token: torch.Tensor,
                          n_prompt: Sequence[int], prompt_feat: torch.Tensor, n_pfeat: Sequence[int], embedding: torch.Tensor,
                          rand_noise: torch.Tensor, flags: int = 0) -> torch.Tensor:
        """One chunk pass for the streams in `slots`: row i of the inputs (shaped as `inference`'s) extends the stream of
        slots[i].  Always streaming=True, finalize=False.  -> mel (n, 80, 2*max(n_token)); row i is valid in
        [:, :2*(n_token[i] - pre_lookahead)] and equals `inference(..., streaming=True, finalize=False)` on utterance i alone.
        flags: 0, or FY_PRECISE on a session opened with precise=True (equal to that call with the same flags; a slot continued in
        the other arithmetic is recomputed in full); FY_DIRECT raises."""
        flags |= FY_STREAMING | FY_NO_FINALIZE
        n = len(slots)
        dev = self.device
        token = token.to(dev, torch.int32).contiguous()
        prompt_token = prompt_token.to(dev, torch.int32).contiguous()
        if prompt_token.shape[1] == 0:
            prompt_token = torch.zeros(n, 1, dtype=torch.int32, device=dev)
        prompt_feat = prompt_feat.to(dev, torch.float32).contiguous()
        if prompt_feat.shape[1] == 0:
            prompt_feat = torch.zeros(n, 1, self.cfg.mel, device=dev)
        embedding = embedding.to(dev, torch.float32).contiguous()
        noise = rand_noise.reshape(self.cfg.mel, -1).to(dev, torch.float32).contiguous()
        assert token.shape[0] == n and prompt_token.shape[0] == n and prompt_feat.shape[0] == n and embedding.shape[0] == n
        frames = 2 * max(int(v) for v in n_token)
        mel = torch.zeros(n, self.cfg.mel, frames, device=dev, dtype=torch.float32)
        check(_lib.lib().fy_flow_infer_streams(self._h, _lib.int_array(slots), n, token.data_ptr(), token.shape[1], _lib.int_array(n_token),
                                               prompt_token.data_ptr(), prompt_token.shape[1], _lib.int_array(n_prompt),
                                               prompt_feat.data_ptr(), prompt_feat.shape[1], _lib.int_array(n_pfeat),
                                               embedding.data_ptr(), noise.data_ptr(), noise.shape[1], mel.data_ptr(), frames,
                                               flags, self._stream()))
        return mel

    def speed(self, mel: torch.Tensor, speed: float) -> torch.Tensor:
        """cli/model.py:435-437: F.interpolate(mel, size=int(F / speed), mode="linear") on (B, 80, F)."""
        mel = mel.to(self.device, torch.float32).contiguous()
        B, C, F = mel.shape
        out = torch.empty(B, C, int(F / speed), device=self.device, dtype=torch.float32)
        check(_lib.lib().fy_mel_speed(mel.data_ptr(), B * C, F, out.data_ptr(), out.shape[2], self._stream()))
        return out

    def estimator(self, x, mask, mu, t, spks, cond, streaming: bool = False, flags: int = 0) -> torch.Tensor:
        """DiT.forward(x, mask, mu, t, spks, cond) on contiguous (B2, 80, T) tensors; returns the result (x is not modified)."""
        out = x.detach().clone().contiguous()
        B2, _, T = out.shape
        if streaming:
            flags |= FY_STREAMING
        check(_lib.lib().fy_dit_estimator(self._h, out.data_ptr(), mask.contiguous().data_ptr() if mask is not None else None,
                                          mu.contiguous().data_ptr(), t.contiguous().data_ptr(), spks.contiguous().data_ptr(),
                                          cond.contiguous().data_ptr(), T, B2, flags, self._stream()))
        return out
