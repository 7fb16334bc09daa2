"""FY_INCREMENTAL on the HiFT vocoder (csrc/hift.hip: hift_infer_incremental): a stream=True call runs the vocoder over the new
mel frames plus a fixed margin and writes only the samples beyond those the stream has delivered.  Those samples must be the
very bits the call without the flag writes there, for every call of a stream, in every precision mode; the work per call must
not grow with the stream; and the stream's life (finalize, stream_reset, a shorter mel, two handles, bad arguments) must hold.
"""
import pytest
import torch

from fangyan_tts_amd import synth
from fangyan_tts_amd._lib import FY_DIRECT, FY_PRECISE, FyError
from fangyan_tts_amd.spec import HiftCfg, ModelCfg
from gpu_util import llm_case, note, synth_mel

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
UP = 480
MARGIN = 37          # the window starts 37 frames before the first sample not yet delivered (CosyVoice3)
MODES = (("bf16", 0), ("direct", FY_DIRECT), ("precise", FY_PRECISE))


def _engine(cfg, max_frames):
    from fangyan_tts_amd.hift import HiftEngine
    sd = synth.state_dict_torch(cfg.manifest(), DEV)
    return sd, HiftEngine(sd, cfg, max_batch=2, max_frames=max_frames, device=DEV)


def _inputs(frames, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    mel = torch.rand(1, 80, frames, generator=g).to(DEV)
    ri = torch.from_numpy(synth.hift_rand_ini()).to(DEV)
    sn = torch.from_numpy(synth.hift_sine_noise(frames * UP)).to(DEV)
    return mel, ri, sn


def _reference_schedule(total, pad=30, hop=50):
    """The facade's mel lengths: a first hop padded to the chunk grid, then 50-frame hops (25 tokens), finalize on the whole."""
    fs, f = [], pad + hop
    while f < total:
        fs.append(f)
        f += hop
    return fs + [total]


def _run_stream(inc, full, mel, ri, sn, schedule, flags, windows=None):
    """Every call of `schedule` (the last one finalizes) on the incremental handle against the plain call on the other handle."""
    inc.stream_reset()
    for i, F in enumerate(schedule):
        fin = i == len(schedule) - 1
        m = mel[:, :, :F].contiguous()
        s_prev = inc.stream_samples()
        w_inc, _ = inc.inference(m, ri, sn, flags=flags, finalize=fin, incremental=True)
        w_full, _ = full.inference(m, ri, sn, flags=flags, finalize=fin)
        s_out = UP * (F if fin else F - 8)
        assert torch.equal(w_inc[:, s_prev:s_out], w_full[:, s_prev:s_out]), (flags, i, F, s_prev, s_out)
        assert not bool(w_inc[:, :s_prev].any()) and not bool(w_inc[:, s_out:].any())      # nothing outside [S_prev, S_out) is written
        assert inc.stream_samples() == (0 if fin else s_out)
        if windows is not None:
            windows.append((F, s_prev, inc.stream_window()))
        if i == 0:
            assert inc.stream_window() == F                                             # a stream's first call computes everything


@pytest.mark.parametrize("mode,flags", MODES)
def test_reference_schedule_bit_identical(mode, flags):
    """The facade's schedule over ~700 frames: every call's new samples equal the whole-mel call's, bit for bit."""
    _, inc = _engine(HiftCfg(), 720)
    _, full = _engine(HiftCfg(), 720)
    mel, ri, sn = _inputs(700)
    voiced = float((full.f0(mel) > HiftCfg().voiced_thr).float().mean())
    note("hift_incremental.json", "voiced_fraction_700", voiced)
    assert 0.05 < voiced < 0.95, voiced                    # both source branches (and the carried phase) are exercised
    wins = []
    _run_stream(inc, full, mel, ri, sn, _reference_schedule(700), flags, wins)
    note("hift_incremental.json", f"reference_schedule.{mode}.windows", wins)


@pytest.mark.parametrize("mode,flags", MODES)
def test_irregular_schedule_bit_identical(mode, flags):
    """Steps of 1, 3 and 9 frames (below the margin), one of several hundred, and a finalize call."""
    _, inc = _engine(HiftCfg(), 720)
    _, full = _engine(HiftCfg(), 720)
    mel, ri, sn = _inputs(700, seed=1)
    _run_stream(inc, full, mel, ri, sn, [20, 21, 24, 33, 90, 91, 94, 103, 450, 451, 500, 700], flags)


@pytest.mark.parametrize("cfg_name", ["tiny", "full"])
def test_long_stream_bit_identical_and_bounded(cfg_name):
    """One stream to the facade's 3200 frames (max_tokens 1600): still bit-identical, and the window of an equal-sized late chunk
    is the same at chunk 5 and at chunk 50 and at most the new frames plus the margin."""
    cfg = HiftCfg() if cfg_name == "full" else HiftCfg.tiny()
    _, inc = _engine(cfg, 3200)
    _, full = _engine(cfg, 3200)
    mel, ri, sn = _inputs(3200, seed=2)
    wins = []
    for mode, flags in MODES:
        wins = []
        _run_stream(inc, full, mel, ri, sn, _reference_schedule(3200), flags, wins)
        note("hift_incremental.json", f"long_stream.{cfg_name}.{mode}.windows", [wins[i] for i in (0, 1, 5, 50, len(wins) - 1)])
    F5, s5, w5 = wins[5]
    F50, s50, w50 = wins[50]
    assert w5 == w50, (wins[5], wins[50])
    assert w5 <= F5 - s5 // UP + MARGIN, wins[5]          # 50 new frames + the 8 the previous chunk held back + the margin
    assert wins[-1][2] < 200 < 3200                        # the finalize call too


def test_lifecycle():
    """Finalize ends the stream; stream_reset mid-stream starts over (equal to a fresh handle); a shorter mel starts over (equal
    to the plain call); two handles keep their own streams."""
    cfg = HiftCfg.tiny()
    _, a = _engine(cfg, 400)
    _, b = _engine(cfg, 400)
    _, plain = _engine(cfg, 400)
    mel, ri, sn = _inputs(400, seed=3)

    def call(h, F, fin=False):
        return h.inference(mel[:, :, :F].contiguous(), ri, sn, finalize=fin, incremental=True)[0]

    def whole(F, fin=False):
        return plain.inference(mel[:, :, :F].contiguous(), ri, sn, finalize=fin)[0]

    a.stream_reset()
    for F in (80, 130, 180):
        call(a, F)
    assert a.stream_samples() == UP * 172 and a.stream_window() < 180
    # finalize ends the stream: the next call starts a new one and computes everything
    w = call(a, 230, fin=True)
    assert a.stream_samples() == 0
    assert torch.equal(w[:, UP * 172:], whole(230, True)[:, UP * 172:])
    w = call(a, 90)
    assert a.stream_window() == 90 and torch.equal(w, whole(90))
    # a shorter mel starts over: the whole call's samples
    call(a, 140)
    assert a.stream_samples() == UP * 132
    w = call(a, 100)
    assert a.stream_window() == 100 and a.stream_samples() == UP * 92 and torch.equal(w, whole(100))
    # stream_reset mid-stream: the same as a fresh handle
    call(a, 150)
    a.stream_reset()
    assert a.stream_samples() == 0
    b.stream_reset()
    for F in (120, 170, 220):
        wa, wb = call(a, F), call(b, F)
        assert torch.equal(wa, wb), F
    # two handles: b's stream is untouched by a's calls, and a fresh handle's first incremental call computes everything
    call(a, 300)
    s_b = b.stream_samples()
    assert s_b == UP * 212
    wb = call(b, 270)
    assert torch.equal(wb[:, s_b: UP * 262], whole(270)[:, s_b: UP * 262])
    _, c = _engine(cfg, 400)
    wc = call(c, 270)
    assert c.stream_window() == 270 and torch.equal(wc, whole(270))


def test_bad_arguments():
    cfg = HiftCfg.tiny()
    _, h = _engine(cfg, 100)
    mel, ri, sn = _inputs(100, seed=4)
    mel2 = torch.cat([mel, mel], 0)
    with pytest.raises(FyError, match="B = 1"):
        h.inference(mel2, ri, sn, finalize=False, incremental=True)
    with pytest.raises(FyError, match="source"):
        h.inference(mel, ri, sn, finalize=False, incremental=True, want_source=True)
    with pytest.raises(FyError, match="at least"):                                      # a chunk shorter than its look-ahead
        h.inference(mel[:, :, :5].contiguous(), ri, sn, finalize=False, incremental=True)
    # the refused calls changed nothing: the next call still begins a new stream
    assert h.stream_samples() == 0
    h.inference(mel, ri, sn, finalize=False, incremental=True)
    assert h.stream_samples() == UP * 92


def _model(cfg, max_tokens, **kw):
    from fangyan_tts_amd.cli.model import CosyVoice3Model
    sd = [synth.state_dict_torch(m.manifest(), DEV, skip=("lm_head",)) for m in (cfg.llm, cfg.flow, cfg.hift)]
    return CosyVoice3Model(sd[0], sd[1], sd[2], cfg, device=DEV, max_batch=1, max_text=64, max_prompt_tokens=32, max_tokens=max_tokens, **kw)


def _chunks_both_ways(m, inp):
    """tts(stream=True) as built (incremental vocoder), then with HiftEngine.inference wrapped to drop `incremental`."""
    inc = [o["tts_speech"] for o in m.tts(**inp, stream=True)]
    window = m.hift.stream_window()
    total = m.last_mel.shape[2]
    orig = m.hift.inference

    def whole(*a, incremental=False, **k):
        return orig(*a, **k)
    m.hift.inference = whole
    try:
        ref = [o["tts_speech"] for o in m.tts(**inp, stream=True)]
    finally:
        del m.hift.inference
    return inc, ref, window, total


def test_facade_stream_equals_whole_vocoder():
    """CosyVoice3Model.tts(stream=True): the chunks equal those of the whole-mel vocoder, at the stream fixtures' size (LM-driven,
    2-3 chunks) and over a long voice-conversion stream (~250 given tokens, ~10 chunks, no LM); the long stream's last vocoder
    call ran over far fewer frames than the stream holds."""
    cfg = ModelCfg.tiny()
    n_text, n_ptext, p_llm, p_flow = 40, 6, 0, 12
    sn = torch.from_numpy(synth.hift_sine_noise(2 * 20 * n_text * UP))
    m = _model(cfg, 20 * n_text, rand_noise=torch.from_numpy(synth.flow_rand_noise(2 * (p_flow + 20 * n_text))),
               rand_ini=torch.from_numpy(synth.hift_rand_ini()), sine_noise=sn)
    t, pt, pk = llm_case(cfg.llm, n_text, n_ptext, p_llm, f"{n_text}_{n_ptext}_{p_llm}_{p_flow}")
    prompt = {
        "flow_prompt_speech_token": torch.from_numpy(synth.randint(f"in.flow.ptoken.{p_flow}", (1, p_flow), 0, 6561)),
        "prompt_speech_feat": torch.from_numpy(synth_mel(f"in.flow.pfeat.{p_flow}", 2 * p_flow)),
        "flow_embedding": torch.from_numpy(synth.normal("in.flow.spk", (1, 192))),
    }
    inp = dict(text=torch.tensor([t], dtype=torch.int32), prompt_text=torch.tensor([pt], dtype=torch.int32),
               llm_prompt_speech_token=torch.tensor([pk], dtype=torch.int32).reshape(1, -1), **prompt)
    inc, ref, _, _ = _chunks_both_ways(m, inp)
    assert len(inc) == len(ref) >= 2
    for i, (a, b) in enumerate(zip(inc, ref)):
        assert torch.equal(a, b), i
    # the long stream: voice conversion (cli/model.py:131-133) - the token list is given
    src = torch.from_numpy(synth.randint("in.vc.source.250", (1, 250), 0, 6561))
    inc, ref, window, total = _chunks_both_ways(m, dict(source_speech_token=src, **prompt))
    note("hift_incremental.json", "facade.vc250", {"chunks": len(inc), "last_window": window, "frames": total})
    assert len(inc) == len(ref) >= 9
    for i, (a, b) in enumerate(zip(inc, ref)):
        assert torch.equal(a, b), i
    assert window < total // 3, (window, total)
