"""The mel store of the vocoder's stream-slot session (csrc/hift.hip: fy_hift_streams_store, fy_hift_stream_slot_push, mel_push_k,
fy_hift_infer_streams with a null mel).  The contract: a stream read from its slot's store gives the very bits the same call gives
when it is handed the concatenated mel as a pointer - compared with torch.equal against a second session that has no store."""
import ctypes as C

import pytest
import torch

from fangyan_tts_amd import _lib, synth
from fangyan_tts_amd._lib import FyError
from fangyan_tts_amd.spec import HiftCfg

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
UP = 480
ERR_ARG, ERR_STATE = "error -1:", "error -4:"


def _engine(cfg, max_frames, max_batch=3):
    from fangyan_tts_amd.hift import HiftEngine
    return HiftEngine(synth.state_dict_torch(cfg.manifest(), DEV), cfg, max_batch=max_batch, max_frames=max_frames, device=DEV)


def _tables(frames):
    return torch.from_numpy(synth.hift_rand_ini()).to(DEV), torch.from_numpy(synth.hift_sine_noise(frames * UP)).to(DEV)


def _mel(total, seed):
    return torch.rand(1, 80, total, generator=torch.Generator(device="cpu").manual_seed(seed)).to(DEV)


def _reference_schedule(total, pad, hop=50):
    """The facade's mel lengths: a first hop padded to the chunk grid, then 50-frame hops (25 tokens), finalize on the whole."""
    fs, f = [], pad + hop
    while f < total:
        fs.append(f)
        f += hop
    return fs + [total]


def _push(eng, rows, poison=7.0):
    """rows: [(slot, mel (1, 80, T), lo, hi)] -> ONE push of frames [lo, hi) of each, laid out as a flow call's output would be:
    an (n, 80, ld) tensor whose row i holds them from an ODD column first[i] on, everything else poisoned."""
    first = [1 + 2 * i for i in range(len(rows))]
    ld = max(f + hi - lo for f, (_, _, lo, hi) in zip(first, rows)) + 3
    src = torch.full((len(rows), 80, ld), poison, device=DEV)
    for i, (_, m, lo, hi) in enumerate(rows):
        src[i, :, first[i]: first[i] + hi - lo] = m[0, :, lo:hi]
    eng.stream_slot_push([r[0] for r in rows], src, first, [hi - lo for _, _, lo, hi in rows])


@pytest.mark.parametrize("tag,totals,cap", [("tiny", (230, 160, 95), 4200), ("full", (180, 130, 95), 192)])
def test_store_reads_equal_pointer_reads(tag, totals, cap):
    """Three ragged streams on the reference chunk schedule.  Every poll pushes the new frames of its streams in ONE launch (two or
    three rows, odd source columns, a row with count 0 for a stream that has nothing new) and vocodes from the stores; a second
    session gets the concatenated mels as pointers.  Every chunk and every finalize call: equal bits.  The tiny case's store has a
    pitch above 4096 frames - the f0 convs' form follows the stream's length, not the pitch."""
    cfg = HiftCfg.tiny() if tag == "tiny" else HiftCfg()
    eng, ref = _engine(cfg, 240), _engine(cfg, 240)
    ri, sn = _tables(240)
    mels = [_mel(t, 50 + i) for i, t in enumerate(totals)]
    plans = [_reference_schedule(t, pad) for t, pad in zip(totals, (30, 10, 0))]
    eng.open_streams(3)
    base = eng.streams_bytes()
    eng.open_streams(3, store_frames=cap)
    assert eng.streams_bytes() - base == 3 * 80 * cap * 4
    ref.open_streams(3)
    assert [eng.stream_slot_frames(s) for s in range(4)] == [0, 0, 0, -1] and ref.stream_slot_frames(0) == 0
    held, zero_rows, multi = [0, 0, 0], 0, 0
    for k in range(max(len(p) for p in plans)):
        live = [i for i in range(3) if k < len(plans[i])]
        idle = [i for i in range(3) if k >= len(plans[i])][:1]              # a stream that ended rides along with count 0
        rows = [(i, mels[i], held[i], plans[i][k]) for i in live] + [(i, mels[i], held[i], held[i]) for i in idle]
        _push(eng, rows)
        zero_rows += len(idle)
        multi += len(rows) >= 2
        for i in live:
            held[i] = plans[i][k]
        assert [eng.stream_slot_frames(s) for s in range(3)] == held
        fins = [k == len(plans[i]) - 1 for i in live]
        got = eng.inference_streams(live, None, ri, sn, fins)
        want = ref.inference_streams(live, [mels[i][:, :, : plans[i][k]] for i in live], ri, sn, fins)
        for i, g, w in zip(live, got, want):
            assert g.shape == w.shape and g.shape[0] > 0 and torch.equal(g, w), (tag, k, i)
            assert eng.stream_slot_samples(i) == ref.stream_slot_samples(i)
    assert zero_rows >= 1 and multi >= 3
    # a reset slot holds nothing and is reused cleanly by another utterance (its stream starts over in both sessions)
    eng.stream_slot_reset(1)
    ref.stream_slot_reset(1)
    assert [eng.stream_slot_frames(s) for s in range(3)] == [held[0], 0, held[2]]
    other = _mel(120, 77)
    for lo, hi, fin in ((0, 60, False), (60, 120, True)):
        _push(eng, [(1, other, lo, hi)])
        got = eng.inference_streams([1], None, ri, sn, [fin])
        want = ref.inference_streams([1], [other[:, :, :hi]], ri, sn, [fin])
        assert torch.equal(got[0], want[0]) and got[0].shape[0] == UP * ((hi if fin else hi - 8) - (0 if lo == 0 else lo - 8))
    # the first frames of a store only (frames below what the slot holds), beside a pointer row in the same call
    eng.stream_slot_reset(0)
    ref.stream_slot_reset(0)
    eng.stream_slot_reset(2)
    ref.stream_slot_reset(2)
    _push(eng, [(0, mels[0], 0, 90)])
    part = mels[2][0, :, :70].contiguous()
    wav, n_new = torch.zeros(2, UP * 90, device=DEV), (C.c_int32 * 2)()
    _lib.check(_lib.lib().fy_hift_infer_streams(eng._h, _lib.int_array([0, 2]), 2, (C.c_void_p * 2)(None, part.data_ptr()), _lib.int_array([80, 70]),
                                                _lib.int_array([80, 70]), _lib.int_array([0, 0]), ri.data_ptr(), sn.data_ptr(), wav.data_ptr(),
                                                UP * 90, n_new, 0, eng._stream()))
    want = ref.inference_streams([0, 2], [mels[0][:, :, :80], mels[2][:, :, :70]], ri, sn, [False, False])
    assert list(n_new) == [UP * 72, UP * 62]
    assert torch.equal(wav[0, : UP * 72], want[0]) and torch.equal(wav[1, : UP * 62], want[1])
    eng.close_streams()
    ref.close_streams()
    assert eng.streams_bytes() == 0 and eng.stream_slot_frames(0) == -1


def test_refusals_leave_the_session_as_it_was():
    cfg = HiftCfg.tiny()
    eng, ref = _engine(cfg, 200, max_batch=2), _engine(cfg, 200, max_batch=2)
    ri, sn = _tables(200)
    a, b = _mel(200, 60), _mel(200, 61)
    src = torch.zeros(2, 80, 64, device=DEV)

    def refused(code, msg, fn):
        before = [(eng.stream_slot_frames(s), eng.stream_slot_samples(s)) for s in range(2)], eng.streams_bytes()
        with pytest.raises(FyError, match=msg) as e:
            fn()
        assert code in str(e.value), str(e.value)
        assert ([(eng.stream_slot_frames(s), eng.stream_slot_samples(s)) for s in range(2)], eng.streams_bytes()) == before

    refused(ERR_STATE, "no stream-slot session", lambda: eng.stream_slot_push([0], src[:1], [0], [10]))
    refused(ERR_STATE, "no stream-slot session", lambda: _lib.check(_lib.lib().fy_hift_streams_store(eng._h, 100)))
    eng.open_streams(2)
    refused(ERR_STATE, "no mel store", lambda: eng.stream_slot_push([0], src[:1], [0], [10]))
    refused(ERR_ARG, "null and the session has no mel store", lambda: eng.inference_streams([0], None, ri, sn, [False], frames=[60]))
    # a store the device cannot give: the byte count is named, the session stays open and usable without one
    refused("error -2:", r"hipMalloc\(%d B\) failed" % (2 * 80 * (1 << 30) * 4), lambda: eng.open_streams(2, store_frames=1 << 30))
    assert eng.stream_slot_frames(0) == 0
    ref.open_streams(2)
    assert torch.equal(eng.inference_streams([0], [a[:, :, :60]], ri, sn, [True])[0], ref.inference_streams([0], [a[:, :, :60]], ri, sn, [True])[0])
    refused(ERR_ARG, "cap_frames 0 below 1", lambda: eng.open_streams(2, store_frames=0))
    eng.open_streams(2, store_frames=100)
    ref.open_streams(2)
    _push(eng, [(0, a, 0, 60), (1, b, 0, 50)])
    got = eng.inference_streams([0, 1], None, ri, sn, [False, False])
    want = ref.inference_streams([0, 1], [a[:, :, :60], b[:, :, :50]], ri, sn, [False, False])
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert [(eng.stream_slot_frames(s), eng.stream_slot_samples(s)) for s in range(2)] == [(60, UP * 52), (50, UP * 42)]
    refused(ERR_ARG, "outside the session's 2 slots", lambda: eng.stream_slot_push([2], src[:1], [0], [10]))
    refused(ERR_ARG, "outside the session's 2 slots", lambda: eng.stream_slot_push([0, -1], src, [0, 0], [10, 10]))
    refused(ERR_ARG, "listed twice", lambda: eng.stream_slot_push([1, 1], src, [0, 0], [10, 10]))
    refused(ERR_ARG, r"3 rows outside \[1, 2\]", lambda: eng.stream_slot_push([0, 1, 0], torch.zeros(3, 80, 64, device=DEV), [0] * 3, [1] * 3))
    refused(ERR_ARG, r"count\[1\] = -1 is negative", lambda: eng.stream_slot_push([0, 1], src, [0, 0], [10, -1]))
    refused(ERR_ARG, r"reads frames \[55, 65\) of a mel of 64", lambda: eng.stream_slot_push([0, 1], src, [0, 55], [10, 10]))
    refused(ERR_ARG, r"reads frames \[-2, 8\)", lambda: eng.stream_slot_push([0], src[:1], [-2], [10]))
    refused(ERR_ARG, "slot 0 would hold 101 frames, the store has room for 100", lambda: eng.stream_slot_push([1, 0], src, [0, 0], [10, 41]))
    refused(ERR_ARG, r"frames\[1\] = 51, slot 1's store holds 50", lambda: eng.inference_streams([0, 1], None, ri, sn, [False, False], frames=[60, 51]))
    refused(ERR_ARG, "listed twice", lambda: eng.inference_streams([0, 0], None, ri, sn, [False, False]))
    # nothing of all that changed a slot: the streams go on, still bit for bit
    _push(eng, [(1, b, 50, 100), (0, a, 60, 100)])
    got = eng.inference_streams([1, 0], None, ri, sn, [True, False])
    want = ref.inference_streams([1, 0], [b[:, :, :100], a[:, :, :100]], ri, sn, [True, False])
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and got[0].shape[0] == UP * 58 and got[1].shape[0] == UP * 40
    # a new store empties every slot; closing frees it
    eng.open_streams(2, store_frames=64)
    assert [eng.stream_slot_frames(s) for s in range(2)] == [0, 0]
    eng.close_streams()
    ref.close_streams()
    assert eng.streams_bytes() == 0
