"""HiFT stream slots (csrc/hift.hip: fy_hift_infer_streams): one incremental vocoder pass over several streams.  The contract is the
single stream's (tests/test_hift_incremental_gpu.py): the samples a call returns for a stream are the very bits a plain whole-mel
`fy_hift_infer` of that stream alone writes at [S_prev, S_out) - compared with torch.equal - whatever the other rows of the call
are doing (another depth, another length, a finalize beside chunks, the other form of the f0 convs).
"""
import ctypes as C

import pytest
import torch

from fangyan_tts_amd import _lib, synth
from fangyan_tts_amd._lib import FY_DIRECT, FY_PRECISE, FyError
from fangyan_tts_amd.hift import stream_new_samples
from fangyan_tts_amd.spec import HiftCfg, ModelCfg
from gpu_util import llm_case, note, synth_mel

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
UP = 480
MARGIN = 37          # a window starts 37 frames before the first sample not yet delivered (CosyVoice3)
MODES = (("bf16", 0), ("direct", FY_DIRECT), ("precise", FY_PRECISE))
SMALL = HiftCfg(base=128, f0_ch=256)     # a reduced config whose synthetic f0 predictor is voiced about half of the time


def _engine(cfg, max_frames, max_batch=4):
    from fangyan_tts_amd.hift import HiftEngine
    sd = synth.state_dict_torch(cfg.manifest(), DEV)
    return HiftEngine(sd, cfg, max_batch=max_batch, max_frames=max_frames, device=DEV)


def _tables(frames):
    return torch.from_numpy(synth.hift_rand_ini()).to(DEV), torch.from_numpy(synth.hift_sine_noise(frames * UP)).to(DEV)


class Stream:
    """One utterance: its mel, and what its stream has delivered so far (kept here, independently of the library)."""

    def __init__(self, total, seed):
        g = torch.Generator(device="cpu").manual_seed(seed)
        self.mel = torch.rand(1, 80, total, generator=g).to(DEV)
        self.total, self.seed, self.delivered, self.last_F = total, seed, 0, 0
        self.windows = []

    def restart(self):
        self.delivered, self.last_F = 0, 0


def _voiced(plain, streams, cfg, key):
    """Both source branches (and the carried phase) must be exercised: no stream is all voiced or all unvoiced."""
    for s in streams:
        v = float((plain.f0(s.mel) > cfg.voiced_thr).float().mean())
        note("hift_stream_slots.json", f"{key}.voiced_fraction.seed{s.seed}_{s.total}", v)
        assert 0.05 < v < 0.95, (s.seed, s.total, v)


def _reference_schedule(total, pad, hop=50):
    """The facade's mel lengths: a first hop padded to the chunk grid, then 50-frame hops (25 tokens), finalize on the whole."""
    fs, f = [], pad + hop
    while f < total:
        fs.append(f)
        f += hop
    return fs + [total]


def poll(eng, plain, ri, sn, items, flags=0):
    """One batched call: items = [(slot, Stream, F, finalize)].  Every stream's new samples against the plain whole-mel call."""
    for slot, s, F, fin in items:
        assert eng.stream_slot_samples(slot) == s.delivered, (slot, F)
        if F < s.last_F:
            s.restart()                                                     # a shorter mel: the call starts the slot's stream over
    got = eng.inference_streams([it[0] for it in items], [s.mel[:, :, :F] for _, s, F, _ in items], ri, sn, [it[3] for it in items],
                                flags=flags)
    assert len(got) == len(items)
    for (slot, s, F, fin), w in zip(items, got):
        want, _ = plain.inference(s.mel[:, :, :F].contiguous(), ri, sn, flags=flags, finalize=fin)
        s_out = UP * (F if fin else F - 8)
        assert w.dim() == 1 and w.shape[0] == stream_new_samples(F, fin, s.delivered) == s_out - s.delivered, (slot, F, fin, w.shape)
        assert torch.equal(w, want[0, s.delivered:s_out]), (flags, slot, s.seed, F, fin, s.delivered)
        assert eng.stream_slot_samples(slot) == (0 if fin else s_out)
        s.windows.append((F, s.delivered, eng.stream_slot_window(slot)))
        if s.delivered == 0:
            assert eng.stream_slot_window(slot) == F                        # a stream's first call computes everything
        s.delivered, s.last_F = (0, 0) if fin else (s_out, F)


@pytest.mark.parametrize("mode,flags", MODES)
def test_ragged_streams_bit_identical(mode, flags):
    """Four streams of different lengths and first-hop pads on the reference schedule, polled together: the calls mix depths, and
    finalize with non-finalize rows, as the shorter streams end while the longer ones go on."""
    cfg = HiftCfg()
    eng, plain = _engine(cfg, 720), _engine(cfg, 720, max_batch=1)
    ri, sn = _tables(700)
    streams = [Stream(700, 0), Stream(430, 11), Stream(180, 12), Stream(95, 13)]
    _voiced(plain, streams, cfg, "ragged")
    plans = [_reference_schedule(s.total, pad) for s, pad in zip(streams, (30, 10, 44, 0))]
    eng.open_streams(4)
    mixed = 0
    for k in range(max(len(p) for p in plans)):
        items = [(i, s, p[k], k == len(p) - 1) for i, (s, p) in enumerate(zip(streams, plans)) if k < len(p)]
        fins = {it[3] for it in items}
        mixed += len(items) > 1 and fins == {True, False}
        poll(eng, plain, ri, sn, items, flags)
    assert mixed >= 2                                                       # finalize rows beside chunk rows, more than once
    wins = streams[0].windows
    note("hift_stream_slots.json", f"ragged.{mode}.windows_stream0", wins)
    (F5, s5, w5), (F9, s9, w9) = wins[5], wins[9]
    assert w5 == w9, (wins[5], wins[9])                                     # equal-sized late chunks: equal windows
    assert w5 <= F5 - s5 // UP + MARGIN, wins[5]                            # 50 new frames + the 8 held back + the margin
    eng.close_streams()


def test_staggered_join_reset_and_reuse():
    """A stream joins while others are mid-stream; a slot is reset mid-stream and reused for another utterance; a slot whose stream
    finalized is reused without a reset.  Every call of every stream still equals its solo whole-mel run (what a fresh handle gives)."""
    cfg = HiftCfg()
    eng, plain = _engine(cfg, 320, max_batch=3), _engine(cfg, 320, max_batch=1)
    ri, sn = _tables(300)
    a, b, c, d = Stream(300, 14), Stream(260, 15), Stream(240, 16), Stream(150, 18)
    _voiced(plain, [a, b, c, d], cfg, "staggered")
    eng.open_streams(3)
    poll(eng, plain, ri, sn, [(0, a, 80, False), (1, b, 60, False)])
    poll(eng, plain, ri, sn, [(0, a, 130, False), (1, b, 110, False)])
    poll(eng, plain, ri, sn, [(0, a, 180, False), (1, b, 160, False), (2, c, 70, False)])      # c joins
    eng.stream_slot_reset(1)                                                                   # b is dropped mid-stream ...
    assert eng.stream_slot_samples(1) == 0 and eng.stream_slot_samples(0) == UP * 172
    poll(eng, plain, ri, sn, [(0, a, 230, False), (1, d, 90, False), (2, c, 120, False)])      # ... and d takes its slot
    poll(eng, plain, ri, sn, [(2, c, 170, False), (1, d, 140, False), (0, a, 300, True)])      # (any order of slots)
    b.restart()
    poll(eng, plain, ri, sn, [(0, b, 60, False), (1, d, 150, True), (2, c, 240, True)])        # b again, in a's finished slot
    poll(eng, plain, ri, sn, [(0, b, 110, False)])
    eng.close_streams()


@pytest.mark.parametrize("mode,flags", MODES)
def test_irregular_steps(mode, flags):
    """Steps of 1, 3 and 9 frames (below the margin), one of several hundred, a slot fed a shorter mel (which starts over), and a
    stream whose only call is a finalize."""
    cfg = HiftCfg()
    eng, plain = _engine(cfg, 540, max_batch=2), _engine(cfg, 540, max_batch=1)
    ri, sn = _tables(520)
    x, y = Stream(520, 17), Stream(150, 18)
    _voiced(plain, [x, y], cfg, "irregular")
    eng.open_streams(2)
    poll(eng, plain, ri, sn, [(0, x, 20, False)], flags)
    poll(eng, plain, ri, sn, [(0, x, 21, False), (1, y, 150, True)], flags)                    # y: a finalize and nothing else
    for F in (24, 33, 42, 400, 401, 404):
        poll(eng, plain, ri, sn, [(0, x, F, False)], flags)
    poll(eng, plain, ri, sn, [(0, x, 100, False)], flags)                                      # shorter: everything again
    assert x.windows[-1] == (100, 0, 100)
    poll(eng, plain, ri, sn, [(0, x, 150, False), (1, y, 60, False)], flags)
    poll(eng, plain, ri, sn, [(0, x, 520, True), (1, y, 61, False)], flags)
    eng.close_streams()


def test_across_the_f0_form_switch():
    """The fp32-MFMA f0 convs sum in another order above 4096 frames.  A stream is taken past that length beside a short one in the
    same calls: each gets the form its own whole length selects, and both stay bit-identical to their solo whole-mel runs.  (The
    call that crosses the switch runs the long stream from frame 0 - its carried phase sums came from the other form - and the
    next one is back on a short window.)"""
    eng, plain = _engine(SMALL, 4300, max_batch=2), _engine(SMALL, 4300, max_batch=1)
    ri, sn = _tables(4200)
    long, short = Stream(4200, 21), Stream(200, 22)
    _voiced(plain, [long, short], SMALL, "form_switch")
    eng.open_streams(2)
    plan_long = [100, 2000, 4000, 4090, 4150, 4200]
    plan_short = [60, 110, 160, 200, 60, 110]
    for k, (Fl, Fs) in enumerate(zip(plan_long, plan_short)):
        if k == 4:
            short.restart()                                                 # (its stream finalized at 200: a new one begins)
        poll(eng, plain, ri, sn, [(0, long, Fl, k == 5), (1, short, Fs, k == 3)])
    assert long.windows[3][2] < 200 and long.windows[4][0] > 4096 and long.windows[5][2] < 200     # short windows on either side
    note("hift_stream_slots.json", "form_switch.windows_long", long.windows)
    eng.close_streams()


def _launches(fn, names=("conv_mfma",)):
    L = _lib.lib()
    L.fy_prof_reset()
    L.fy_prof_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        L.fy_prof_enable(0)
    out = {k: _lib.prof_get(k)[2] for k in names}
    L.fy_prof_reset()
    return out


def test_one_launch_chain_per_call():
    """A call that continues four streams records the conv launches of ONE single-stream incremental call - not four times as many."""
    cfg = HiftCfg.tiny()
    eng, one = _engine(cfg, 200), _engine(cfg, 200, max_batch=1)
    ri, sn = _tables(200)
    streams = [Stream(200, 30 + i) for i in range(4)]
    m0 = streams[0].mel
    one.stream_reset()
    one.inference(m0[:, :, :80].contiguous(), ri, sn, finalize=False, incremental=True)
    single = _launches(lambda: one.inference(m0[:, :, :130].contiguous(), ri, sn, finalize=False, incremental=True))
    eng.open_streams(4)
    eng.inference_streams([0, 1, 2, 3], [s.mel[:, :, :F] for s, F in zip(streams, (80, 70, 90, 60))], ri, sn, [False] * 4)
    four = _launches(lambda: eng.inference_streams([0, 1, 2, 3], [s.mel[:, :, :F] for s, F in zip(streams, (130, 120, 140, 110))], ri, sn,
                                                   [False] * 4))
    eng.close_streams()
    assert single["conv_mfma"] > 10, single
    assert four == single, (four, single)


def _raw_call(eng, slots, mels, fins, ri, sn, wav_ld):
    """fy_hift_infer_streams with a wav pitch of the caller's choosing (the Python mirror always sizes it right)."""
    n = len(slots)
    ms = [m[0].contiguous() for m in mels]
    fr = [int(m.shape[1]) for m in ms]
    wav = torch.zeros(n, max(wav_ld, 1), device=DEV)
    n_new = (C.c_int32 * n)()
    rc = _lib.lib().fy_hift_infer_streams(eng._h, _lib.int_array(slots), n, (C.c_void_p * n)(*[m.data_ptr() for m in ms]), _lib.int_array(fr),
                                          _lib.int_array(fr), _lib.int_array([int(f) for f in fins]), ri.data_ptr(), sn.data_ptr(),
                                          wav.data_ptr(), wav_ld, n_new, 0, eng._stream())
    return rc, _lib.lib().fy_last_error().decode()


def test_errors_and_lifecycle():
    cfg = HiftCfg.tiny()
    eng, plain = _engine(cfg, 100, max_batch=2), _engine(cfg, 400, max_batch=1)
    ri, sn = _tables(400)
    a, b = Stream(400, 40), Stream(400, 41)
    args = lambda s, F: s.mel[:, :, :F]
    with pytest.raises(FyError, match="session"):                            # no session open
        eng.inference_streams([0], [args(a, 60)], ri, sn, [False])
    assert eng.streams_bytes() == 0 and eng.stream_slot_samples(0) == -1
    for bad in (0, 3):
        with pytest.raises(FyError, match="slots outside"):
            eng.open_streams(bad)
    eng.open_streams(2)
    assert 0 < eng.streams_bytes() < 1 << 20
    poll(eng, plain, ri, sn, [(0, a, 60, False)])
    with pytest.raises(FyError, match="outside the session"):               # a slot out of range
        eng.inference_streams([2], [args(b, 60)], ri, sn, [False])
    with pytest.raises(FyError, match="listed twice"):
        eng.inference_streams([0, 0], [args(a, 90), args(a, 90)], ri, sn, [False, False])
    with pytest.raises(FyError, match="3 streams in a session of 2"):        # n > n_slots
        eng.inference_streams([0, 1, 0], [args(a, 90)] * 3, ri, sn, [False] * 3)
    with pytest.raises(FyError, match=r"outside \[1, 0\]"):                   # frames outside [1, mel_ld]
        eng.inference_streams([0, 1], [args(a, 90), args(b, 0)], ri, sn, [False, False])
    with pytest.raises(FyError, match="at least 9 frames"):                  # a chunk shorter than its look-ahead
        eng.inference_streams([0, 1], [args(a, 90), args(b, 5)], ri, sn, [False, False])
    with pytest.raises(FyError, match="need 300 frame rows"):                # 2 rows x a 150-frame window > 2 x 100
        eng.inference_streams([0, 1], [args(a, 90), args(b, 150)], ri, sn, [False, False])
    rc, msg = _raw_call(eng, [0, 1], [args(a, 90), args(b, 60)], [False, False], ri, sn, wav_ld=UP * 52 - 1)
    assert rc != 0
    assert "wav_ld" in msg and str(UP * 52) in msg, msg                       # (slot 1 brings 52 frames of samples, slot 0 only 30)
    # the refused calls changed nothing: both slots are where they were, and the next call is still bit-identical
    assert eng.stream_slot_samples(0) == UP * 52 and eng.stream_slot_samples(1) == 0
    poll(eng, plain, ri, sn, [(0, a, 90, False), (1, b, 60, False)])
    # a single 200-frame window fits the two rows' buffers (2 x 100 frame rows)
    b.restart()
    eng.stream_slot_reset(1)
    poll(eng, plain, ri, sn, [(1, b, 200, True)])
    # close / reopen: the session's bytes go and come back, the slots start fresh
    eng.close_streams()
    assert eng.streams_bytes() == 0
    eng.close_streams()                                                     # (closing twice is harmless)
    eng.open_streams(1)
    assert eng.streams_bytes() > 0 and eng.stream_slot_samples(0) == 0 and eng.stream_slot_samples(1) == -1
    a.restart()
    poll(eng, plain, ri, sn, [(0, a, 70, False)])
    # the single-stream API on the same handle, beside the open session
    eng.stream_reset()
    w1, _ = eng.inference(b.mel[:, :, :60].contiguous(), ri, sn, finalize=False, incremental=True)
    poll(eng, plain, ri, sn, [(0, a, 100, False)])
    w2, _ = eng.inference(b.mel[:, :, :100].contiguous(), ri, sn, finalize=False, incremental=True)
    assert eng.stream_samples() == UP * 92 and eng.stream_window() < 100
    want1, _ = plain.inference(b.mel[:, :, :60].contiguous(), ri, sn, finalize=False)
    want2, _ = plain.inference(b.mel[:, :, :100].contiguous(), ri, sn, finalize=False)
    assert torch.equal(w1[:, : UP * 52], want1[:, : UP * 52]) and torch.equal(w2[:, UP * 52: UP * 92], want2[:, UP * 52: UP * 92])
    poll(eng, plain, ri, sn, [(0, a, 100, True)])
    eng.close_streams()
    assert eng.streams_bytes() == 0


def test_facade_one_vocoder_pass_per_poll():
    """tts_stream_batch over K = 3 utterances: per stream, chunk by chunk, the tensors `tts(stream=True)` yields for that utterance
    alone; and the lane has built no per-stream vocoder engines."""
    from fangyan_tts_amd.cli.model import CosyVoice3Model
    cfg = ModelCfg.tiny()
    cases = [(40, 6, 0, 12), (30, 5, 0, 25), (24, 4, 0, 7)]
    sd = [synth.state_dict_torch(m.manifest(), DEV, skip=("lm_head",)) for m in (cfg.llm, cfg.flow, cfg.hift)]
    n_text_max = max(c[0] for c in cases)
    m = CosyVoice3Model(sd[0], sd[1], sd[2], cfg, device=DEV, max_batch=len(cases), max_text=64, max_prompt_tokens=32, max_tokens=20 * n_text_max,
                        rand_noise=torch.from_numpy(synth.flow_rand_noise(2 * (32 + 20 * n_text_max))),
                        rand_ini=torch.from_numpy(synth.hift_rand_ini()), sine_noise=torch.from_numpy(synth.hift_sine_noise(2 * 20 * n_text_max * UP)))
    inputs = []
    for n_text, n_ptext, p_llm, p_flow in cases:
        ctag = f"sb.{n_text}_{n_ptext}_{p_llm}_{p_flow}"
        t, pt, pk = llm_case(cfg.llm, n_text, n_ptext, p_llm, ctag)
        inputs.append({
            "text": torch.tensor([t], dtype=torch.int32), "prompt_text": torch.tensor([pt], dtype=torch.int32),
            "llm_prompt_speech_token": torch.tensor([pk], dtype=torch.int32).reshape(1, -1),
            "flow_prompt_speech_token": torch.from_numpy(synth.randint(f"in.flow.ptoken.sb.{p_flow}", (1, p_flow), 0, 6561)),
            "prompt_speech_feat": torch.from_numpy(synth_mel(f"in.flow.pfeat.sb.{p_flow}", 2 * p_flow)),
            "flow_embedding": torch.from_numpy(synth.normal(f"in.flow.spk.sb.{p_flow}", (1, 192))),
        })
    alone = [[o["tts_speech"] for o in m.tts(**inp, stream=True)] for inp in inputs]
    got = [[] for _ in inputs]
    for i, o in m.tts_stream_batch(inputs):
        got[i].append(o["tts_speech"])
    for i in range(len(inputs)):
        assert len(got[i]) == len(alone[i]) >= 2, i
        for k, (x, y) in enumerate(zip(got[i], alone[i])):
            assert x.device.type == "cpu" and x.shape == y.shape and torch.equal(x, y), (i, k)
    assert all("stream_hifts" not in ln.__dict__ for ln in m.lanes)
    assert all(ln.hift.streams_bytes() == 0 for ln in m.lanes)               # the session is closed with the call
