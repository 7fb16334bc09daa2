"""Host side of the speech-token LM: mirrors `CosyVoice3LM.inference`
(CosyVoice/cosyvoice/llm/llm.py:713-748) plus the token filter of
`CosyVoiceModel.llm_job` (cli/model.py:101-129) over the C ABI, for a batch."""
from __future__ import annotations

import ctypes as C
from collections import deque
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import check
from .spec import LlmCfg


def _cfg_struct(cfg: LlmCfg, weight_planes: int = 0) -> _lib.LlmConfig:
    c = _lib.LlmConfig()
    _lib.lib().fy_llm_default_config(C.byref(c))
    c.hidden, c.layers, c.q_heads, c.kv_heads, c.head_dim = cfg.hidden, cfg.layers, cfg.q_heads, cfg.kv_heads, cfg.head_dim
    c.inter, c.vocab, c.speech_tokens, c.rms_eps, c.rope_theta = cfg.inter, cfg.vocab, cfg.speech_tokens, cfg.rms_eps, cfg.rope_theta
    c.weight_planes = weight_planes
    return c


def _fill_slots(free: Sequence[int], pending: deque) -> List[Tuple[int, int]]:
    """The slot policy: requests in arrival order into the lowest free slots -> [(request, slot)]."""
    return [(pending.popleft(), s) for s in sorted(free)[: len(pending)]]


def plan_slots(raw_lengths: Sequence[int], n_slots: int, steps_per_poll: int = 8):
    """The schedule `LlmEngine.generate_continuous` runs when request r emits exactly raw_lengths[r] tokens (a forced length,
    min_len == max_len): a pure function of the lengths, no GPU.  Requests enter the lowest free slots in arrival order; the join
    emits a request's first token, so it needs raw_lengths[r] - 1 token steps; every poll runs `steps_per_poll` token steps while
    any slot is occupied, then the slots whose request has ended are released and refilled.
    -> (token_steps, joins): the number of token steps issued, and [(token steps issued before the join, [(request, slot), ...])]."""
    assert n_slots >= 1 and steps_per_poll >= 1 and all(int(n) >= 1 for n in raw_lengths)
    pending = deque(range(len(raw_lengths)))
    left: Dict[int, int] = {}                 # slot -> token steps its request still needs
    t, joins = 0, []
    while pending or left:
        batch = _fill_slots([s for s in range(n_slots) if s not in left], pending)
        if batch:
            joins.append((t, batch))
            for r, s in batch:
                left[s] = int(raw_lengths[r]) - 1
        t += steps_per_poll
        left = {s: n - steps_per_poll for s, n in left.items() if n > steps_per_poll}
    return t, joins


def grouped_steps(raw_lengths: Sequence[int], n_slots: int, steps_per_poll: int = 8) -> int:
    """Token steps of the schedule without slots: arrival-order groups of n_slots, each run to its longest request (its first
    token comes from the prefill), the stop flags looked at every steps_per_poll steps."""
    t = 0
    for g in range(0, len(raw_lengths), n_slots):
        need = max(int(n) for n in raw_lengths[g: g + n_slots]) - 1
        t += max(1, -(-need // steps_per_poll)) * steps_per_poll
    return t


class ServeSchedule:
    """Every decision of the serving loop (`CosyVoice3Model.tts_serve`), as host state without a GPU: which request joins which
    slot, and which retired requests form the next flow group.  `plan_serve` drives it with forced lengths, `tts_serve` with what
    the device reports; neither decides anything else.  One poll is: `arrive` for the requests that came in, `join`, the token
    steps (the caller's), `retire` for the slots seen ended, `cut`, `next_poll`."""

    def __init__(self, n_slots: int, group_max: int, group_wait: int):
        assert n_slots >= 1 and group_max >= 1 and group_wait >= 0
        self.n_slots, self.group_max, self.group_wait = int(n_slots), int(group_max), int(group_wait)
        self.pending: deque = deque()             # requests that arrived and hold no slot yet, in arrival order
        self.occupied: Dict[int, int] = {}        # slot -> request
        self.ready: List[Tuple[int, int, int]] = []   # (request, length, poll it retired in), oldest first
        self.poll = 0

    def arrive(self, request: int):
        self.pending.append(request)

    def join(self) -> List[Tuple[int, int]]:
        """The poll's one join: waiting requests in arrival order into the lowest free slots -> [(request, slot)]."""
        batch = _fill_slots([s for s in range(self.n_slots) if s not in self.occupied], self.pending)
        self.occupied.update({s: r for r, s in batch})
        return batch

    def retire(self, ended: Dict[int, int]) -> List[Tuple[int, int]]:
        """ended: {slot seen ended in this poll: its token count}.  The slots are free again; their requests enter the ready
        list in ascending slot order -> [(request, slot)] in that order."""
        out = []
        for s in sorted(ended):
            r = self.occupied.pop(s)
            self.ready.append((r, int(ended[s]), self.poll))
            out.append((r, s))
        return out

    def drop(self, request: int):
        """Take a retired request out of the ready list (it cannot be decoded: no token)."""
        self.ready = [e for e in self.ready if e[0] != request]

    def cut(self, more_coming: bool) -> List[Tuple[int, ...]]:
        """The flow groups this poll forms, oldest first: `group_max` ready requests make a group; what is left goes as one
        group once its oldest member has waited `group_wait` polls, or once nothing is running, waiting for a slot or still to
        arrive.  Inside a group the longest comes first (requests of equal length in retirement order)."""
        groups = []
        while len(self.ready) >= self.group_max:
            groups.append(self.ready[: self.group_max])
            self.ready = self.ready[self.group_max:]
        if self.ready and (self.poll - self.ready[0][2] >= self.group_wait or not (self.occupied or self.pending or more_coming)):
            groups.append(self.ready)
            self.ready = []
        return [tuple(r for r, _, _ in sorted(g, key=lambda e: -e[1])) for g in groups]

    def next_poll(self):
        self.poll += 1

    @property
    def idle(self) -> bool:
        return not (self.pending or self.occupied or self.ready)


def plan_serve(n_tokens: Sequence[int], arrivals: Optional[Sequence[int]], n_slots: int, steps_per_poll: int = 8, group_max: int = 8,
               group_wait: int = 2, lengths: Optional[Sequence[int]] = None):
    """The schedule `CosyVoice3Model.tts_serve` runs when request r arrives in poll arrivals[r] (non-decreasing; None: all in
    poll 0; the input ends with its last arrival) and emits exactly n_tokens[r] tokens (as `plan_slots`: the join emits the first,
    so it needs n_tokens[r] - 1 token steps; a request that ends on a stop token needs one step more than it emits).  lengths:
    the counts the groups are sorted by (after the silent-token filter); default n_tokens.  A pure function, no GPU.
    Poll p: the requests with arrivals[r] <= p wait for a slot; ONE join puts them into the lowest free slots in arrival order;
    `steps_per_poll` token steps run if any slot is occupied; the slots seen ended are exported and released, their requests wait
    in the ready list; `ServeSchedule.cut` forms the flow groups.
    -> one dict per poll: {"poll", "joins": [(request, slot)], "steps", "retired": [(request, slot)], "groups": [(request, ...)]}.
    With every request present at poll 0 the token steps (the sum of "steps") are `plan_slots`' for the same lengths."""
    N = len(n_tokens)
    arrivals = [0] * N if arrivals is None else [int(a) for a in arrivals]
    lengths = n_tokens if lengths is None else lengths
    assert len(arrivals) == N and len(lengths) == N and steps_per_poll >= 1 and all(int(n) >= 1 for n in n_tokens)
    assert all(a >= 0 for a in arrivals) and all(arrivals[i] <= arrivals[i + 1] for i in range(N - 1)), "arrival polls in request order"
    sch = ServeSchedule(n_slots, group_max, group_wait)
    left: Dict[int, int] = {}                 # slot -> token steps its request still needs
    nxt, polls = 0, []
    while nxt < N or not sch.idle:
        while nxt < N and arrivals[nxt] <= sch.poll:
            sch.arrive(nxt)
            nxt += 1
        joins = sch.join()
        for r, s in joins:
            left[s] = int(n_tokens[r]) - 1
        steps = steps_per_poll if sch.occupied else 0
        ended = {}
        if steps:
            ended = {s: int(lengths[sch.occupied[s]]) for s, n in left.items() if n <= steps_per_poll}
            left = {s: n - steps_per_poll for s, n in left.items() if n > steps_per_poll}
        retired = sch.retire(ended)
        groups = sch.cut(nxt < N)
        polls.append({"poll": sch.poll, "joins": joins, "steps": steps, "retired": retired, "groups": groups})
        sch.next_poll()
    return polls


class LlmEngine:
    """weights: the llm.pt state_dict (reference key names, fp32 CUDA tensors; lm_head not needed).
    weight_planes: 0 (default) = the library chooses - two bf16 planes per matrix (w = hi + lo) exactly when some weight is not
    bf16-representable, as in a real checkpoint (the reference runs llm.pt in fp32, cli/cosyvoice.py:193), else one; 1 / 2 force it."""

    def __init__(self, weights: Dict[str, torch.Tensor], cfg: LlmCfg = LlmCfg(), max_batch: int = 8, max_ctx: int = 1024,
                 device: Optional[torch.device] = None, keep_weights: bool = False, weight_planes: int = 0):
        self.cfg = cfg
        self._weight_planes = weight_planes
        self.device = device or next(iter(weights.values())).device
        self.max_batch, self.max_ctx = max_batch, max_ctx
        self._h = C.c_void_p()
        weights = {k: v for k, v in weights.items() if "lm_head" not in k}
        self._weights = weights if keep_weights else None          # needed only for load_state_dict
        self._peers = []          # other handles built from the same weights (a model's extra LM handles and lanes): they follow load_state_dict
        self._create(weights)

    def _create(self, weights):
        arr, keep = _lib.tensor_table(weights)
        cs = _cfg_struct(self.cfg, self._weight_planes)
        with torch.cuda.device(self.device):
            check(_lib.lib().fy_llm_create(C.byref(self._h), C.byref(cs), arr, len(weights), self.max_batch, self.max_ctx, self._stream()))
        del keep

    def load_state_dict(self, state_dict, strict: bool = True):
        """torch.nn.Module.load_state_dict's contract for the keys of llm.pt (compare_inference.py:36-43 swaps a
        fine-tuned LM in with strict=False): the engine is rebuilt from the merged weights."""
        if self._weights is None:
            raise RuntimeError("LlmEngine was built without keep_weights=True; it cannot merge a partial state_dict")
        known = set(self._weights) | {"llm.model.lm_head.weight"}
        unexpected = [k for k in state_dict if k not in known]
        missing = [k for k in self._weights if k not in state_dict]
        if strict and (unexpected or missing):
            raise RuntimeError(f"Error(s) in loading state_dict: missing {missing[:5]}, unexpected {unexpected[:5]}")
        for k, v in state_dict.items():
            if k in self._weights:
                if tuple(v.shape) != tuple(self._weights[k].shape):
                    raise RuntimeError(f"size mismatch for {k}: {tuple(v.shape)} vs {tuple(self._weights[k].shape)}")
                self._weights[k] = v.detach().to(self.device, torch.float32).contiguous()
        for e in [self] + list(self._peers):                      # every handle that was built from these weights
            e.close()
            e._create(self._weights)
        return missing, unexpected

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def close(self):
        if self._h:
            _lib.lib().fy_llm_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _pack_ids(text, prompt_text, prompt_speech, min_len, max_len, min_ratio, max_ratio):
        B = len(text)
        ids, n_all, ps, n_ps = [], [], [], []
        for b in range(B):
            ids += list(prompt_text[b]) + list(text[b])
            n_all.append(len(prompt_text[b]) + len(text[b]))
            ps += list(prompt_speech[b])
            n_ps.append(len(prompt_speech[b]))
        mn = [int(len(text[b]) * min_ratio) for b in range(B)] if min_len is None else list(min_len)
        mx = [int(len(text[b]) * max_ratio) for b in range(B)] if max_len is None else list(max_len)
        return (_lib.int_array(ids), _lib.int_array(n_all), _lib.int_array(ps or [0]), _lib.int_array(n_ps), _lib.int_array(mn),
                _lib.int_array(mx)), mx

    def _pack(self, text, prompt_text, prompt_speech, min_len, max_len, min_ratio, max_ratio):
        B = len(text)
        arrays, mx = self._pack_ids(text, prompt_text, prompt_speech, min_len, max_len, min_ratio, max_ratio)
        out_ld = max(mx)
        out = torch.zeros(B, out_ld, dtype=torch.int32, device=self.device)
        out_n = torch.zeros(B, dtype=torch.int32, device=self.device)
        raw_n = torch.zeros(B, dtype=torch.int32, device=self.device)
        return (*arrays, B, out.data_ptr(), out_ld), out, out_n, raw_n

    def generate(self, text: Sequence[Sequence[int]], prompt_text: Sequence[Sequence[int]],
                 prompt_speech: Sequence[Sequence[int]], min_len: Optional[Sequence[int]] = None,
                 max_len: Optional[Sequence[int]] = None, min_ratio: float = 2, max_ratio: float = 20):
        """Per-sequence python lists of ids -> (out_ids (B, max(max_len)) int32 CUDA, out_n (B) CUDA, raw_n (B) CUDA).
        min/max default to llm.py:743-744 (2x / 20x the text-only length)."""
        args, out, out_n, raw_n = self._pack(text, prompt_text, prompt_speech, min_len, max_len, min_ratio, max_ratio)
        check(_lib.lib().fy_llm_generate(self._h, *args, out_n.data_ptr(), raw_n.data_ptr(), 0, self._stream()))
        return out, out_n, raw_n

    def begin(self, text, prompt_text, prompt_speech, min_len=None, max_len=None, min_ratio: float = 2, max_ratio: float = 20):
        """The generator form of `inference` (llm.py:511-525 yields ids one by one): prefill + the first token.  Returns
        (out_ids, out_n, raw_n) as `generate`; they fill up as `step` is called."""
        args, out, out_n, raw_n = self._pack(text, prompt_text, prompt_speech, min_len, max_len, min_ratio, max_ratio)
        check(_lib.lib().fy_llm_begin(self._h, *args, self._stream()))
        self._gen = (out, out_n, raw_n, len(text))
        return out, out_n, raw_n

    def prefill_embeds(self, embeds: Sequence[torch.Tensor], min_len: Sequence[int], max_len: Sequence[int]):
        """The embeddings-level entry - the reference's vLLM hand-off (llm.py:482-510 passes `prompt_embeds` = lm_input (L, 896)
        per request): the caller has assembled lm_input itself.  embeds: one (L_b, hidden) CUDA tensor per sequence, fp32 or
        bf16 (all alike).  Prefill + the first token; `step` continues.  Returns (out_ids, out_n, raw_n) as `begin`."""
        B = len(embeds)
        dt = embeds[0].dtype
        assert dt in (torch.float32, torch.bfloat16) and all(e.dtype == dt and e.dim() == 2 and e.shape[1] == self.cfg.hidden for e in embeds)
        rows = torch.cat([e.to(self.device) for e in embeds], dim=0).contiguous()
        out_ld = max(int(m) for m in max_len)
        out = torch.zeros(B, out_ld, dtype=torch.int32, device=self.device)
        out_n = torch.zeros(B, dtype=torch.int32, device=self.device)
        raw_n = torch.zeros(B, dtype=torch.int32, device=self.device)
        check(_lib.lib().fy_llm_prefill(self._h, rows.data_ptr(), 0 if dt == torch.float32 else 1, _lib.int_array([e.shape[0] for e in embeds]),
                                        _lib.int_array(min_len), _lib.int_array(max_len), B, out.data_ptr(), out_ld, self._stream()))
        self._gen = (out, out_n, raw_n, B)
        return out, out_n, raw_n

    # ---- decode slots: sequences join and leave between token steps (fy_llm_slots_open ...) ----
    def open_slots(self, out_ld: Optional[int] = None):
        """Start a slot session: all `max_batch` slots free.  Returns (out_ids (max_batch, out_ld), out_n, raw_n), CUDA int32,
        indexed by slot; they fill up as `join` and `step` are called.  out_ld defaults to max_ctx (no sequence can emit more)."""
        out_ld = int(out_ld or self.max_ctx)
        out = torch.zeros(self.max_batch, out_ld, dtype=torch.int32, device=self.device)
        out_n = torch.zeros(self.max_batch, dtype=torch.int32, device=self.device)
        raw_n = torch.zeros(self.max_batch, dtype=torch.int32, device=self.device)
        check(_lib.lib().fy_llm_slots_open(self._h, out.data_ptr(), out_ld, self._stream()))
        self._gen = (out, out_n, raw_n, self.max_batch)
        return out, out_n, raw_n

    def join(self, slots: Sequence[int], text, prompt_text, prompt_speech, min_len=None, max_len=None, min_ratio: float = 2,
             max_ratio: float = 20):
        """Prefill new sequences (arguments as `begin`) into the free slots `slots` and sample their first tokens; the slots
        already running are untouched and go on at the next `step`."""
        arrays, _ = self._pack_ids(text, prompt_text, prompt_speech, min_len, max_len, min_ratio, max_ratio)
        check(_lib.lib().fy_llm_slot_join(self._h, _lib.int_array(slots), len(slots), *arrays, self._stream()))

    def join_embeds(self, slots: Sequence[int], embeds: Sequence[torch.Tensor], min_len: Sequence[int], max_len: Sequence[int]):
        """`join` from embedding rows (as `prefill_embeds`): the reference's `add_request(uuid, prompt_embeds, SamplingParams)`."""
        dt = embeds[0].dtype
        assert dt in (torch.float32, torch.bfloat16) and all(e.dtype == dt and e.dim() == 2 and e.shape[1] == self.cfg.hidden for e in embeds)
        rows = torch.cat([e.to(self.device) for e in embeds], dim=0).contiguous()
        check(_lib.lib().fy_llm_slot_join_embeds(self._h, _lib.int_array(slots), len(slots), rows.data_ptr(), 0 if dt == torch.float32 else 1,
                                                 _lib.int_array([e.shape[0] for e in embeds]), _lib.int_array(min_len), _lib.int_array(max_len),
                                                 self._stream()))
        del rows                                             # the caching allocator keeps it for the stream's queued work

    def release(self, slot: int):
        """Free a slot, ended or not (a cancelled request)."""
        check(_lib.lib().fy_llm_slot_release(self._h, int(slot), self._stream()))

    def export(self, slots: Sequence[int], ld: Optional[int] = None):
        """The ids of the occupied slots `slots` as one ragged batch for `FlowEngine.inference` (fy_llm_slots_export: one copy
        kernel on the current stream, no host copy of the id matrix) -> (tokens (len(slots), ld) int32 CUDA, a fresh tensor whose
        row i holds slot slots[i]'s ids and zeros beyond them; counts, a host list).  ld defaults to the session's out_ld; a row
        with more than ld ids is cut to ld and its count says so.  The slots may be released and joined again at once."""
        n = len(slots)
        if ld is None:                                       # (no session: the library says so)
            ld = self._gen[0].shape[1] if getattr(self, "_gen", None) else 1
        ld = int(ld)
        tokens = torch.empty(max(n, 1), max(ld, 1), dtype=torch.int32, device=self.device)
        counts = torch.empty(max(n, 1), dtype=torch.int32, device=self.device)
        host = (C.c_int32 * max(n, 1))()
        check(_lib.lib().fy_llm_slots_export(self._h, _lib.int_array(slots), n, tokens.data_ptr(), ld, counts.data_ptr(), host, self._stream()))
        return tokens, list(host)

    def live(self) -> List[int]:
        """The occupied slots of the session (running, or ended and not yet released)."""
        state = (C.c_int32 * self.max_batch)()
        _lib.lib().fy_llm_slots_live(self._h, state)
        return [s for s in range(self.max_batch) if state[s]]

    @property
    def slot_steps(self) -> int:
        """Token steps launched since `open_slots`."""
        return int(_lib.lib().fy_llm_slots_steps(self._h))

    def generate_continuous(self, text, prompt_text, prompt_speech, min_len: Optional[Sequence[int]] = None,
                            max_len: Optional[Sequence[int]] = None, steps_per_poll: int = 8, min_ratio: float = 2, max_ratio: float = 20):
        """Any number of requests (more than max_batch too) through the slots, in arrival order: join into the lowest free slots,
        `steps_per_poll` token steps, collect and release the slots that ended, refill - the schedule `plan_slots` computes.
        -> (ids, raw_n): per request the emitted ids (silent-token filter applied, as `generate`) and the count before the filter."""
        N = len(text)
        mn = [int(len(t) * min_ratio) for t in text] if min_len is None else list(min_len)
        mx = [int(len(t) * max_ratio) for t in text] if max_len is None else list(max_len)
        out, out_n, raw_n = self.open_slots(max(mx))
        pending, occupied = deque(range(N)), {}
        ids: List[Optional[List[int]]] = [None] * N
        raw = [0] * N
        while pending or occupied:
            batch = _fill_slots([s for s in range(self.max_batch) if s not in occupied], pending)
            if batch:
                rs = [r for r, _ in batch]
                self.join([s for _, s in batch], [text[r] for r in rs], [prompt_text[r] for r in rs], [prompt_speech[r] for r in rs],
                          min_len=[mn[r] for r in rs], max_len=[mx[r] for r in rs])
                occupied.update({s: r for r, s in batch})
            n, fin = self.step(steps_per_poll)
            ended = [s for s in occupied if fin[s]]
            if ended:
                host, rn = out.cpu(), raw_n.cpu().tolist()
                for s in ended:
                    r = occupied.pop(s)
                    ids[r], raw[r] = host[s, : n[s]].tolist(), rn[s]
                    self.release(s)
        return ids, raw

    def step(self, n_steps: int):
        """Up to `n_steps` more tokens for the sequences still running -> (tokens kept so far per sequence, finished flags).
        In a slot session both lists have max_batch entries, indexed by slot (free slots: 0, True)."""
        out, out_n, raw_n, B = self._gen
        fin = (C.c_int32 * B)()
        check(_lib.lib().fy_llm_step(self._h, int(n_steps), out.data_ptr(), out.shape[1], out_n.data_ptr(), raw_n.data_ptr(), fin,
                                     self._stream()))
        return out_n.cpu().tolist(), [bool(f) for f in fin]

    def set_sampler(self, kind: str = "greedy", uniforms: Optional[torch.Tensor] = None, top_k: int = 25, top_p: float = 0.8,
                    win_size: int = 10, tau_r: float = 0.1):
        """"greedy" (SURVEY 8 a4 rule) or "ras": the reference's default repetition-aware sampling (utils/common.py:137-166,
        parameters of cosyvoice3.yaml) with torch.multinomial's draws replaced by the inverse CDF at `uniforms`
        (float32 CUDA (max_batch, n), one row per sequence, consumed from the start at every generate call)."""
        if kind == "greedy":
            check(_lib.lib().fy_llm_set_sampler(self._h, 0, None, 0, top_k, top_p, win_size, tau_r))
            self._uniforms = None
            return
        assert kind == "ras" and uniforms is not None and uniforms.is_cuda and uniforms.dtype == torch.float32
        u = uniforms.reshape(-1, uniforms.shape[-1]).contiguous()
        assert u.shape[0] >= self.max_batch, "one row of uniforms per sequence slot"
        self._uniforms = u                                   # borrowed by the library until the next call
        check(_lib.lib().fy_llm_set_sampler(self._h, 1, u.data_ptr(), u.shape[1], top_k, top_p, win_size, tau_r))

    def set_decode_mode(self, persistent):
        """True / 1 (default): one persistent launch per token step (lowest latency; for <= 8 sequences it holds most of the chip).
        False / 0: one launch per operation, whose short kernels interleave with other streams.
        2: only the few-CU persistent step (any batch <= 32) - what tts_pipeline uses beside its flow decoders."""
        check(_lib.lib().fy_llm_set_decode_mode(self._h, int(persistent)))

    @property
    def persistent(self) -> bool:
        return bool(_lib.lib().fy_llm_decode_mode(self._h))

    @property
    def decode_mode(self) -> int:
        """0, 1 or 2 as set_decode_mode takes them (0 also when the handle has no persistent step for the mode asked for)."""
        return int(_lib.lib().fy_llm_decode_mode(self._h))

    @property
    def weight_planes(self) -> int:
        return int(_lib.lib().fy_llm_weight_planes(self._h))

    def logp(self, step: int, B: int) -> torch.Tensor:
        buf = torch.empty(B, self.cfg.n_speech, device=self.device)
        check(_lib.lib().fy_llm_logp(self._h, step, buf.data_ptr(), self._stream()))
        return buf
