"""Packed rows (FY_PACKED, csrc/flow.hip): a ragged `fy_flow_infer` batch sends only its valid rows through the DiT blocks.

The bar is BIT-IDENTITY with the padded call on the same handle and the same batch, over every utterance's valid frames
F_b = 2 * (n_token[b] - look): the same Tmax, so attention takes the same workgroup form; a row's sums in a product depend neither
on M nor on the rows beside it; LayerNorm-modulate is per row; the rotary epilogue reads the same table values through a table
with one row per compact row.  No tolerance anywhere.  `FlowEngine.last_rows` tells which path ran: 2 B Tmax padded, 2 sum(T) =
`flow.packed_rows(T)[1]` packed.  Never against a solo run: that has another Tmax and may take the other attention form.
"""
import pytest
import torch

from fangyan_tts_amd import _lib, synth
from fangyan_tts_amd.spec import FlowCfg, ModelCfg
from gpu_util import llm_case, maxerr, note, synth_mel

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LOOK = 3
TINY_CASES = [(20, 10), (24, 0), (9, 4), (1, 0)]             # T = 60, 48, 26, 2: sequence starts off every tile boundary
FULL_CASES = [(150, 20), (60, 0), (129, 20), (3, 0)]         # T = 340 (past 256: the other tiling rule), 120, 298, 6 (< a 32-query block)


class Batch:
    """(n_token, n_prompt) per utterance -> the padded input tensors of one `inference` call."""

    def __init__(self, cfg, cases, tag):
        self.cases = cases
        self.n = [n for n, _ in cases]
        self.p = [p for _, p in cases]
        B, Nm, Pm = len(cases), max(self.n), max(max(self.p), 1)
        self.token = torch.zeros(B, Nm, dtype=torch.int32)
        self.ptoken = torch.zeros(B, Pm, dtype=torch.int32)
        self.pfeat = torch.zeros(B, 2 * Pm, 80)
        for b, (n, p) in enumerate(cases):
            self.token[b, :n] = torch.from_numpy(synth.randint(f"in.flow.token.pk.{tag}.{b}", (1, n), 0, cfg.vocab))[0]
            if p:
                self.ptoken[b, :p] = torch.from_numpy(synth.randint(f"in.flow.ptoken.pk.{tag}.{b}", (1, p), 0, cfg.vocab))[0]
                self.pfeat[b, : 2 * p] = torch.from_numpy(synth_mel(f"in.flow.pfeat.pk.{tag}.{b}", 2 * p))[0]
        self.emb = torch.from_numpy(synth.normal(f"in.flow.spk.pk.{tag}", (B, cfg.spk_in)))
        self.noise = torch.from_numpy(synth.flow_rand_noise(2 * max(n + p for n, p in cases)))

    def rows(self, look=0):
        return [2 * (n + p - look) for n, p in self.cases]

    def run(self, eng, **kw):
        return eng.inference(self.token, self.n, self.ptoken, self.p, self.pfeat, [2 * p for p in self.p], self.emb, self.noise, **kw)


def parity(eng, batch, tag, flags=0, streaming=False, finalize=True):
    """padded against packed on the same handle: the row counts of both calls, then every utterance's valid frames bit for bit"""
    from fangyan_tts_amd.flow import packed_rows
    look = 0 if finalize else LOOK
    T = batch.rows(look)
    want = batch.run(eng, flags=flags, streaming=streaming, finalize=finalize)
    assert eng.last_rows == 2 * len(T) * max(T), (tag, eng.last_rows)
    got = batch.run(eng, flags=flags, streaming=streaming, finalize=finalize, packed=True)
    assert eng.last_rows == 2 * sum(T) == packed_rows(T)[1], (tag, eng.last_rows, T)
    assert got.shape == want.shape
    for b, n in enumerate(batch.n):
        F = 2 * (n - look)
        assert bool(want[b, :, :F].abs().max() > 0), (tag, b)
        assert torch.equal(got[b, :, :F], want[b, :, :F]), (tag, b, maxerr(got[b, :, :F], want[b, :, :F]))


def make(cfg, max_batch, max_frames, unrounded=False):
    from fangyan_tts_amd.flow import FlowEngine
    if unrounded:
        with synth.unrounded_weights():
            sd = synth.state_dict_torch(cfg.manifest(), DEV)
    else:
        sd = synth.state_dict_torch(cfg.manifest(), DEV)
    return FlowEngine(sd, cfg, max_batch=max_batch, max_frames=max_frames, device=DEV)


@pytest.fixture(scope="module")
def tiny():
    return make(FlowCfg.tiny(), 4, 320)


@pytest.fixture(scope="module")
def full():
    return make(FlowCfg(), 4, 340)


def test_abi_last_rows_and_layout(tiny):
    from fangyan_tts_amd.flow import FlowEngine, packed_rows
    L = _lib.lib()
    assert hasattr(L, "fy_flow_last_rows") and _lib.FY_PACKED == 32
    assert int(L.fy_flow_last_rows(None)) == -1
    fresh = make(FlowCfg.tiny(), 2, 64)
    assert fresh.last_rows == 0                                         # before any call
    fresh.close()
    import inspect
    assert "packed" in inspect.signature(FlowEngine.inference).parameters
    batch = Batch(tiny.cfg, TINY_CASES, "abi")
    T = batch.rows()
    assert T == [60, 48, 26, 2]
    batch.run(tiny)
    assert tiny.last_rows == 2 * 4 * 60
    batch.run(tiny, packed=True)
    assert tiny.last_rows == 2 * sum(T) == packed_rows(T)[1] == 272
    # one utterance, or equal lengths: the padded path, whose row count is the same
    one = Batch(tiny.cfg, TINY_CASES[:1], "abi1")
    one.run(tiny, packed=True)
    assert tiny.last_rows == 2 * 60
    same = Batch(tiny.cfg, [(20, 10), (30, 0), (16, 14)], "abi3")
    same.run(tiny, packed=True)
    assert tiny.last_rows == 2 * 3 * 60


@pytest.mark.parametrize("mode", ["full_attention", "streaming", "streaming_chunk"])
def test_tiny_default_arithmetic(tiny, mode):
    cases = list(TINY_CASES)
    if mode == "streaming_chunk":
        cases[3] = (1 + LOOK, 0)                                        # the shortest utterance a chunk call takes: 2 rows again
    batch = Batch(tiny.cfg, cases, mode)
    parity(tiny, batch, mode, streaming=mode != "full_attention", finalize=mode != "streaming_chunk")


@pytest.mark.parametrize("flag", ["FY_PRECISE", "FY_DIRECT"])
def test_tiny_precise_and_direct(tiny, flag):
    parity(tiny, Batch(tiny.cfg, TINY_CASES, flag), flag, flags=getattr(_lib, flag))


@pytest.mark.parametrize("mode", ["default", "precise", "chunk_mask"])
def test_full_size(full, mode):
    """FlowCfg() at max_batch 4, 340 frames.  default: the LayerNorm fold runs when the handle built its tables (recorded in
    the notes file flow_packed.json; a handle created with too little free memory runs the unfolded chain, and the comparison holds the
    same way)."""
    batch = Batch(full.cfg, FULL_CASES, "full")
    assert batch.rows() == [340, 120, 298, 6]
    if mode == "default":
        note("flow_packed.json", "full.default.ln_fold", bool(full.ln_fold))
    parity(full, batch, mode, flags=_lib.FY_PRECISE if mode == "precise" else 0, streaming=mode == "chunk_mask")


def test_two_weight_planes_precise():
    """Weights that are not bf16-representable: FY_PRECISE multiplies by both planes (and runs the position convolutions on the fp32
    kernel); packed against padded on that handle."""
    eng = make(FlowCfg.tiny(), 4, 64, unrounded=True)
    assert eng.weight_planes == 2
    parity(eng, Batch(eng.cfg, TINY_CASES, "fp32w"), "fp32w", flags=_lib.FY_PRECISE)
    eng.close()


class Stream:
    """One stream=True utterance on the reference's chunk schedule (25-token hops, 25 prompt tokens: no first-hop pad)."""
    P, HOP = 25, 25

    def __init__(self, cfg, tag):
        self.token = torch.from_numpy(synth.randint(f"in.flow.token.pk.st.{tag}", (1, 3 * self.HOP + LOOK), 0, cfg.vocab))
        self.ptoken = torch.from_numpy(synth.randint(f"in.flow.ptoken.pk.st.{tag}", (1, self.P), 0, cfg.vocab))
        self.pfeat = torch.from_numpy(synth_mel(f"in.flow.pfeat.pk.st.{tag}", 2 * self.P))
        self.emb = torch.from_numpy(synth.normal(f"in.flow.spk.pk.st.{tag}", (1, cfg.spk_in)))
        self.noise = torch.from_numpy(synth.flow_rand_noise(2 * (self.P + 3 * self.HOP)))

    def args(self, k):
        n = k * self.HOP + LOOK
        return (self.token[:, :n].contiguous(), [n], self.ptoken, [self.P], self.pfeat, [2 * self.P], self.emb, self.noise)

    def valid(self, k):
        return 2 * k * self.HOP


def test_state_incremental_stream_and_slot_session(tiny):
    """A packed call touches neither the single incremental stream's state nor an open stream-slot session: between two chunks it
    behaves as the padded call does."""
    eng, cfg = tiny, tiny.cfg
    u = Stream(cfg, "a")
    ragged = Batch(cfg, TINY_CASES, "state")
    whole = [eng.inference(*u.args(k), streaming=True, finalize=False) for k in (1, 2)]
    seen = {}
    for packed in (False, True):
        eng.stream_reset()
        first = eng.inference(*u.args(1), streaming=True, finalize=False, incremental=True)
        assert eng.last_rows == 2 * 2 * (u.P + u.HOP)
        assert torch.equal(first[:, :, : u.valid(1)], whole[0][:, :, : u.valid(1)])
        ragged.run(eng, packed=packed)
        assert eng.last_rows == (272 if packed else 480)
        second = eng.inference(*u.args(2), streaming=True, finalize=False, incremental=True)
        seen[packed] = (eng.stream_rows(), eng.last_rows)
        assert torch.equal(second[:, :, : u.valid(2)], whole[1][:, :, : u.valid(2)]), packed      # still the whole recompute
    assert seen[True] == seen[False], seen
    # an open stream-slot session: slot 0 continued after a packed call equals the uninterrupted run
    w = Stream(cfg, "b")
    cap = 2 * (w.P + 3 * w.HOP)
    outs = {}
    for packed in (None, True):
        eng.open_streams(2, cap)
        try:
            eng.stream_slot_reset(0)
            eng.inference_streams([0], *w.args(1))
            if packed:
                ragged.run(eng, packed=True)
                assert eng.last_rows == 272
            assert eng.stream_slot_rows(0) == 2 * (w.P + w.HOP)
            outs[packed] = eng.inference_streams([0], *w.args(2))
            assert eng.stream_slot_rows(0) == 2 * (w.P + 2 * w.HOP)
        finally:
            eng.close_streams()
    assert torch.equal(outs[True], outs[None])
    assert torch.equal(outs[True][:, :, : w.valid(2)], eng.inference(*w.args(2), streaming=True, finalize=False)[:, :, : w.valid(2)])


def model_inputs(cfg, cases, tag):
    inputs = []
    for n_text, n_ptext, p_llm, p_flow in cases:
        ctag = f"pk.{tag}.{n_text}_{n_ptext}_{p_llm}_{p_flow}"
        t, pt, pk = llm_case(cfg.llm, n_text, n_ptext, p_llm, ctag)
        inputs.append({
            "text": torch.tensor([t], dtype=torch.int32), "prompt_text": torch.tensor([pt], dtype=torch.int32),
            "llm_prompt_speech_token": torch.tensor([pk], dtype=torch.int32).reshape(1, -1),
            "flow_prompt_speech_token": torch.from_numpy(synth.randint(f"in.flow.ptoken.{ctag}", (1, p_flow), 0, 6561)),
            "prompt_speech_feat": torch.from_numpy(synth_mel(f"in.flow.pfeat.{ctag}", 2 * p_flow)),
            "flow_embedding": torch.from_numpy(synth.normal(f"in.flow.spk.{ctag}", (1, 192))),
        })
    return inputs


@pytest.fixture(scope="module")
def model():
    from fangyan_tts_amd.cli.model import CosyVoice3Model
    cfg = ModelCfg.tiny()
    sd = [synth.state_dict_torch(m.manifest(), DEV, skip=("lm_head",)) for m in (cfg.llm, cfg.flow, cfg.hift)]
    max_tokens = 160
    return CosyVoice3Model(sd[0], sd[1], sd[2], cfg, device=DEV, max_batch=3, max_text=64, max_prompt_tokens=32, max_tokens=max_tokens,
                           rand_noise=torch.from_numpy(synth.flow_rand_noise(2 * (32 + max_tokens))),
                           rand_ini=torch.from_numpy(synth.hift_rand_ini()),
                           sine_noise=torch.from_numpy(synth.hift_sine_noise(2 * max_tokens * 480)))


def test_model_batch_and_pipeline(model):
    """flow_packed = True: the same wav, sample counts and tokens from tts_batch and from a tts_pipeline of two batches; lengths forced
    ragged through min_len = max_len."""
    m = model
    assert m.flow_packed is False
    ins = model_inputs(m.cfg, [(8, 6, 0, 12), (6, 5, 0, 25), (7, 4, 0, 7)], "b")
    lens = [40, 21, 9]
    batches, blens = [ins, ins[::-1]], [lens, [13, 30, 22]]
    got = {}
    for packed in (False, True):
        m.flow_packed = packed
        try:
            wav, samples, toks = m.tts_batch(ins, min_len=lens, max_len=lens)
            rows = m.lanes[0].flow.last_rows
            pipe = list(m.tts_pipeline(batches, min_len=blens, max_len=blens))
        finally:
            m.flow_packed = False
        got[packed] = (wav, samples, toks, pipe, rows)
    n_tok = [t.numel() for t in got[False][2]]                          # what the LM kept of the forced lengths (silent-token filter)
    T = [2 * (n + p) for n, p in zip(n_tok, (12, 25, 7))]
    assert len(set(T)) == 3, T
    assert got[False][4] == 2 * 3 * max(T) and got[True][4] == 2 * sum(T), (got[False][4], got[True][4], T)
    assert got[True][1] == got[False][1]
    assert torch.equal(got[True][0], got[False][0])
    assert all(torch.equal(a, b) for a, b in zip(got[True][2], got[False][2]))
    assert len(got[True][3]) == len(got[False][3]) == 2
    for (w1, s1, t1), (w0, s0, t0) in zip(got[True][3], got[False][3]):
        assert s1 == s0 and torch.equal(w1, w0) and all(torch.equal(a, b) for a, b in zip(t1, t0))


def test_model_stream_batch_final_group(model):
    """tts_stream_batch of 3 streams, two of which end in the same poll: the same chunks bit for bit with flow_packed, and the final
    group of two went through the packed path."""
    m = model
    ins = model_inputs(m.cfg, [(8, 6, 0, 25), (6, 5, 0, 25), (7, 4, 0, 25)], "s")
    # 25 tokens per poll, chunks of 25 + 3 look-ahead tokens: 80 tokens end in poll 5, 60 and 70 tokens both in poll 4
    forced = [80, 60, 70]
    seen, rows = {}, {}
    flow, llm = m.lanes[0].flow, m.lanes[0].llm
    join = llm.join
    llm.join = lambda slots, text, ptext, pspeech: join(slots, text, ptext, pspeech, min_len=[forced[i] for i in slots], max_len=[forced[i] for i in slots])
    try:
        for packed in (False, True):
            m.flow_packed = packed
            calls = []
            orig = flow.inference

            def tap(*a, **kw):
                r = orig(*a, **kw)
                calls.append((list(a[1]), list(a[3]), flow.last_rows))
                return r
            flow.inference = tap
            try:
                got = [[] for _ in ins]
                for i, o in m.tts_stream_batch(ins):
                    got[i].append(o["tts_speech"])
            finally:
                del flow.inference
                m.flow_packed = False
            seen[packed], rows[packed] = got, calls
    finally:
        del llm.join
    for i in range(3):
        assert len(seen[False][i]) >= 2, i
        assert [c.shape[1] for c in seen[True][i]] == [c.shape[1] for c in seen[False][i]], i
        assert all(torch.equal(a, b) for a, b in zip(seen[True][i], seen[False][i])), i
    groups = [c for c in rows[True] if len(c[0]) > 1]
    assert groups, rows[True]                                           # two streams did end in the same poll
    for (n, p, r), (n0, p0, r0) in zip(rows[True], rows[False]):
        T = [2 * (a + b) for a, b in zip(n, p)]
        assert (n, p) == (n0, p0) and r0 == 2 * len(T) * max(T)
        assert r == (2 * sum(T) if len(set(T)) > 1 else 2 * len(T) * max(T)), (n, p, r)
    assert any(len(set(2 * (a + b) for a, b in zip(c[0], c[1]))) > 1 for c in groups), groups      # ... at different lengths
