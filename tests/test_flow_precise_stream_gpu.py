"""The fp32-class (FY_PRECISE) flow decoder on the streaming side: incremental chunks of one stream (fy_flow_infer with
FY_INCREMENTAL) and stream slots (fy_flow_infer_streams), csrc/flow.hip.

The contract is the default mode's (tests/test_flow_stream_slots_gpu.py), with no tolerance: for every chunk of every stream the
valid mel frames under FY_PRECISE are `torch.equal` to the full FY_PRECISE recompute of that stream alone - `inference(...,
streaming=True, finalize=False, flags=FY_PRECISE)` at B = 1 on a second engine.  Row by row the split path runs what
dit_forward(..., FY_PRECISE) runs: gemm_split has one tiling per shape whatever M is, LayerNorm-modulate and the convolutions are
per row, and the split attention walks a kept query's keys in the whole-sequence launch's 64-key tiles from key 0.  Full-size
FlowCfg(), synthetic weights, the reference's chunk schedule: 25-token hops, 3 look-ahead tokens, the first hop padded so that
prompt + hop is a multiple of 25 tokens.  Every full recompute is computed once and shared (REF).  A slot session takes FY_PRECISE
once it is opened with precise=True (fy_flow_streams_precise); a plain session refuses the flag, as it always has.
"""
import pytest
import torch

from fangyan_tts_amd import _lib, synth
from fangyan_tts_amd._lib import FY_DIRECT, FY_PRECISE
from fangyan_tts_amd.spec import FlowCfg, ModelCfg
from gpu_util import llm_case, maxerr, synth_mel

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HOP, LOOK = 25, 3
K_MAX, P_MAX = 5, 50
N_MAX = K_MAX * HOP + 24 + LOOK + 4                       # tokens of the longest call (the largest first-hop pad, an off-boundary tail)
CAP = 2 * (N_MAX + P_MAX)


class Utt:
    """One utterance's inputs; n_in(k) = tokens of its k-th chunk call (k = 1, 2, ...)."""

    def __init__(self, tag, p_tok, cfg):
        self.tag, self.p_tok = tag, p_tok
        self.token = torch.from_numpy(synth.randint(f"in.flow.token.pslots.{tag}", (1, N_MAX), 0, cfg.vocab))
        self.ptoken = torch.from_numpy(synth.randint(f"in.flow.ptoken.pslots.{tag}", (1, max(p_tok, 1)), 0, cfg.vocab))[:, :p_tok]
        self.pfeat = torch.from_numpy(synth_mel(f"in.flow.pfeat.pslots.{tag}", 2 * max(p_tok, 1)))[:, :2 * p_tok]
        self.emb = torch.from_numpy(synth.normal(f"in.flow.spk.pslots.{tag}", (1, cfg.spk_in)))
        self.pad = -(-p_tok // HOP) * HOP - p_tok

    def n_in(self, k):
        return k * HOP + self.pad + LOOK

    def rows(self, n_in):
        return 2 * (self.p_tok + n_in - LOOK)

    def args(self, n_in, noise):
        return (self.token[:, :n_in].contiguous(), [n_in], self.ptoken, [self.p_tok], self.pfeat, [2 * self.p_tok], self.emb, noise)


def make_engines(cfg, sd):
    from fangyan_tts_amd.flow import FlowEngine
    eng = FlowEngine(sd, cfg, max_batch=1, max_frames=CAP, device=DEV)
    ref = FlowEngine(sd, cfg, max_batch=1, max_frames=CAP, device=DEV)
    noise = torch.from_numpy(synth.flow_rand_noise(CAP))
    return cfg, eng, ref, noise, {}


@pytest.fixture(scope="module")
def engines():
    cfg = FlowCfg()
    return make_engines(cfg, synth.state_dict_torch(cfg.manifest(), DEV))


def full(E, u, n_in, flags=FY_PRECISE):
    """The stream alone, everything recomputed, on the second engine - once per (utterance, length, mode)."""
    cfg, eng, ref, noise, REF = E
    key = (u.tag, u.p_tok, n_in, flags)
    if key not in REF:
        REF[key] = ref.inference(*u.args(n_in, noise), streaming=True, finalize=False, flags=flags)
    return REF[key]


def batched(E, calls, flags=FY_PRECISE):
    """calls: [(slot, Utt, n_in)] -> mel (n, 80, frames) of one inference_streams call."""
    cfg, eng, ref, noise, _ = E
    n = len(calls)
    Nm, Pm = max(c[2] for c in calls), max(max(c[1].p_tok for c in calls), 1)
    token = torch.zeros(n, Nm, dtype=torch.int32)
    ptoken = torch.zeros(n, Pm, dtype=torch.int32)
    pfeat = torch.zeros(n, 2 * Pm, 80)
    emb = torch.cat([c[1].emb for c in calls])
    for i, (_, u, n_in) in enumerate(calls):
        token[i, :n_in] = u.token[0, :n_in]
        ptoken[i, :u.p_tok] = u.ptoken[0]
        pfeat[i, :2 * u.p_tok] = u.pfeat[0]
    return eng.inference_streams([c[0] for c in calls], token, [c[2] for c in calls], ptoken, [c[1].p_tok for c in calls],
                                 pfeat, [2 * c[1].p_tok for c in calls], emb, noise, flags=flags)


def poll(E, calls, flags=FY_PRECISE, keeps=None):
    """One batched call; every listed stream against its own full recompute in the same mode, then the rows each slot keeps."""
    eng = E[1]
    mel = batched(E, calls, flags)
    for i, (slot, u, n_in) in enumerate(calls):
        valid = 2 * (n_in - LOOK)
        want = full(E, u, n_in, flags)
        assert torch.equal(mel[i, :, :valid], want[0, :, :valid]), (slot, u.tag, n_in, flags, maxerr(mel[i, :, :valid], want[0, :, :valid]))
        keep = u.rows(n_in) if keeps is None else keeps[i]
        assert eng.stream_slot_rows(slot) == keep, (slot, n_in)
    return mel


def profiled(fn, names=("gemm_split", "dit_attention_split", "conv_mfma", "gemm_bf16", "dit_attention")):
    """{name: (work, launches)} of the profiled launches fn() issues."""
    L = _lib.lib()
    L.fy_prof_reset()
    L.fy_prof_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        L.fy_prof_enable(0)
    out = {k: _lib.prof_get(k)[1:] for k in names}
    L.fy_prof_reset()
    return out


def poll_profiled(E, calls, flags=FY_PRECISE):
    """poll() under the launch profiler; the references are computed first, so only the batched call's launches are counted."""
    for _, u, n_in in calls:
        full(E, u, n_in, flags)
    torch.cuda.synchronize()
    return profiled(lambda: poll(E, calls, flags))


def split_work(cfg, front_rows, block_rows):
    """The algorithmic work gemm_split reports (4 M N K per product, one weight plane) for a chunk pass whose input projection runs
    over front_rows rows and whose blocks see block_rows rows."""
    D, C, inner, FF = cfg.dim, cfg.mel, cfg.heads * cfg.head_dim, cfg.dim * cfg.ff_mult
    per_row = cfg.depth * (3 * inner * D + D * inner + FF * D + D * FF) + C * D
    return 4.0 * cfg.n_timesteps * (front_rows * D * 4 * C + block_rows * per_row)


@pytest.mark.parametrize("p_tok", [50, 13])
def test_single_stream_incremental_chunks(engines, p_tok):
    """fy_flow_infer(FY_INCREMENTAL | FY_PRECISE): every chunk equals the full precise recompute and its rows are kept; a call that
    ends off the chunk boundary is computed whole and keeps nothing, and the call after it starts over."""
    cfg, eng, ref, noise, _ = engines
    u = Utt(f"s{p_tok}", p_tok, cfg)
    eng.stream_reset()
    for k in range(1, 5):
        n_in = u.n_in(k)
        inc = eng.inference(*u.args(n_in, noise), streaming=True, finalize=False, incremental=True, flags=FY_PRECISE)
        valid = 2 * (n_in - LOOK)
        want = full(engines, u, n_in)
        assert torch.equal(inc[:, :, :valid], want[:, :, :valid]), (k, maxerr(inc[:, :, :valid], want[:, :, :valid]))
        assert eng.stream_rows() == u.rows(n_in), k          # the call really was incremental: its rows are kept
    off = u.n_in(2) + 4
    inc = eng.inference(*u.args(off, noise), streaming=True, finalize=False, incremental=True, flags=FY_PRECISE)
    assert torch.equal(inc, full(engines, u, off))
    assert eng.stream_rows() == 0
    n_in = u.n_in(3)
    inc = eng.inference(*u.args(n_in, noise), streaming=True, finalize=False, incremental=True, flags=FY_PRECISE)
    assert torch.equal(inc, full(engines, u, n_in))
    assert eng.stream_rows() == u.rows(n_in)


def test_single_stream_forgotten_reset(engines):
    """A caller that forgets stream_reset between two utterances: the handle keeps 150 precise rows of a 25-token prompt on a chunk
    boundary, and the next precise call brings another prompt length and MORE rows than are kept (200).  It cannot be an extension:
    the call starts over - every row through the blocks and through the attention - equals the full recompute, and its rows are
    kept for the chunk after it.  Then fewer tokens than the stream holds: starts over as well."""
    cfg, eng, ref, noise, _ = engines
    u1, u2 = Utt("r25", 25, cfg), Utt("r50", 50, cfg)
    run = lambda u, k: eng.inference(*u.args(u.n_in(k), noise), streaming=True, finalize=False, incremental=True, flags=FY_PRECISE)
    eng.stream_reset()
    for k in (1, 2):
        assert torch.equal(run(u1, k), full(engines, u1, u1.n_in(k)))
    assert eng.stream_rows() == u1.rows(u1.n_in(2)) == 150
    for k in (2, 3, 1):                                                          # 200 rows (> 150 kept), 250 (extends), 150 (shrinks)
        got = {}
        w = profiled(lambda: got.update(mel=run(u2, k)))
        valid = 2 * (u2.n_in(k) - LOOK)
        want = full(engines, u2, u2.n_in(k))
        assert torch.equal(got["mel"][:, :, :valid], want[:, :, :valid]), (k, maxerr(got["mel"][:, :, :valid], want[:, :, :valid]))
        T = u2.rows(u2.n_in(k))
        assert eng.stream_rows() == T, k
        new = 2 * HOP if k == 3 else T                                           # frames whose rows went through the blocks
        assert w["gemm_split"][0] == pytest.approx(split_work(cfg, 2 * T, 2 * new), rel=1e-9), (k, w)
    # the same with another count of prompt FRAMES only (prompt tokens equal): the kept rows are not this stream's either
    a = list(u2.args(u2.n_in(2), noise))
    a[4], a[5] = u2.pfeat[:, :96].contiguous(), [96]
    mel = eng.inference(*a, streaming=True, finalize=False, incremental=True, flags=FY_PRECISE)
    assert torch.equal(mel, ref.inference(*a, streaming=True, finalize=False, flags=FY_PRECISE))
    assert eng.stream_rows() == u2.rows(u2.n_in(2))


def test_single_stream_mode_switch_and_direct(engines):
    """The handle records the arithmetic of its kept rows: a call in the other one starts over and keeps its own rows (the work of
    its products says how many rows went through the blocks); FY_PRECISE | FY_DIRECT keeps the full recompute and breaks the stream."""
    cfg, eng, ref, noise, _ = engines
    u = Utt("s50", 50, cfg)
    eng.stream_reset()
    run = lambda k, flags: eng.inference(*u.args(u.n_in(k), noise), streaming=True, finalize=False, incremental=True, flags=flags)
    T = [None] + [u.rows(u.n_in(k)) for k in range(1, 5)]
    assert torch.equal(run(1, 0), full(engines, u, u.n_in(1), 0))
    got = {}
    w = profiled(lambda: got.update(mel=run(2, FY_PRECISE)))                 # default rows kept: the precise call computes all of its rows
    assert torch.equal(got["mel"], full(engines, u, u.n_in(2))) and eng.stream_rows() == T[2]
    assert w["gemm_split"][0] == pytest.approx(split_work(cfg, 2 * T[2], 2 * T[2]), rel=1e-9) and w["gemm_bf16"][1] == 0, w
    w = profiled(lambda: got.update(mel=run(3, FY_PRECISE)))                 # ... and the next one only the new rows
    assert torch.equal(got["mel"], full(engines, u, u.n_in(3))) and eng.stream_rows() == T[3]
    assert w["gemm_split"][0] == pytest.approx(split_work(cfg, 2 * T[3], 2 * (T[3] - T[2])), rel=1e-9), w
    assert w["dit_attention_split"][1] == cfg.n_timesteps * cfg.depth and w["dit_attention"][1] == 0, w
    assert torch.equal(run(4, 0), full(engines, u, u.n_in(4), 0)) and eng.stream_rows() == T[4]      # back: starts over in the default mode
    mel = run(2, FY_PRECISE | FY_DIRECT)
    assert torch.equal(mel, ref.inference(*u.args(u.n_in(2), noise), streaming=True, finalize=False, flags=FY_PRECISE | FY_DIRECT))
    assert eng.stream_rows() == 0


def test_ragged_slots_equal_full_recompute(engines):
    cfg, eng, ref, noise, _ = engines
    utts = [Utt("a", 50, cfg), Utt("b", 40, cfg), Utt("c", 13, cfg)]                      # 40 and 13: padded first hops
    eng.open_streams(3, CAP, precise=True)
    try:
        for s in range(3):
            eng.stream_slot_reset(s)
        for k in range(1, 4):
            poll(engines, [(s, u, u.n_in(k)) for s, u in enumerate(utts)])
    finally:
        eng.close_streams()
    assert eng.streams_bytes == 0


def test_staggered_joins_and_mode_switches(engines):
    cfg, eng, ref, noise, _ = engines
    A, B, D = Utt("a", 50, cfg), Utt("b", 40, cfg), Utt("d", 37, cfg)
    eng.open_streams(3, CAP, precise=True)
    try:
        eng.stream_slot_reset(0)
        poll(engines, [(0, A, A.n_in(1))])
        poll(engines, [(0, A, A.n_in(2))])
        eng.stream_slot_reset(1)                                                  # B joins while A is at chunk 3
        poll(engines, [(0, A, A.n_in(3)), (1, B, B.n_in(1))])
        eng.stream_slot_reset(0)                                                  # A has ended: D takes its slot
        assert eng.stream_slot_rows(0) == 0
        poll(engines, [(0, D, D.n_in(1))])
        # slot 0 goes on in the precise mode, slot 1 in the default mode, in separate calls: B's first default call finds precise
        # rows and recomputes the stream, its second extends it; all of them equal the default full recompute
        poll(engines, [(1, B, B.n_in(2))], flags=0)
        poll(engines, [(0, D, D.n_in(2))])
        w = poll_profiled(engines, [(1, B, B.n_in(3))], flags=0)
        assert w["gemm_split"][1] == 0 and w["dit_attention"][1] == cfg.n_timesteps * cfg.depth, w
        # one precise call for both: slot 1 (default rows) is recomputed in full and keeps its rows, slot 0 beside it stays incremental
        calls = [(0, D, D.n_in(3)), (1, B, B.n_in(4))]
        w = poll_profiled(engines, calls)
        Tp = max(D.rows(D.n_in(3)), B.rows(B.n_in(4)))
        new = 2 * (D.rows(D.n_in(3)) - D.rows(D.n_in(2))) + 2 * B.rows(B.n_in(4))
        assert w["gemm_split"][0] == pytest.approx(split_work(cfg, 4 * Tp, new), rel=1e-9) and w["gemm_bf16"][1] == 0, w
        w = poll_profiled(engines, [(1, B, B.n_in(5)), (0, D, D.n_in(4))])      # both incremental now
        Tp = max(D.rows(D.n_in(4)), B.rows(B.n_in(5)))
        assert w["gemm_split"][0] == pytest.approx(split_work(cfg, 4 * Tp, 4 * 2 * HOP), rel=1e-9), w
    finally:
        eng.close_streams()


def test_one_launch_chain_per_poll(engines):
    """A precise call that advances 3 streams by a chunk each issues, inside the (step, block) loops, the launches of a precise call
    for 1 stream - not 3 times as many."""
    cfg, eng, ref, noise, _ = engines
    utts = [Utt("a", 50, cfg), Utt("b", 40, cfg), Utt("c", 13, cfg)]
    eng.open_streams(3, CAP, precise=True)
    try:
        eng.stream_slot_reset(0)
        batched(engines, [(0, utts[0], utts[0].n_in(1))])
        one = profiled(lambda: batched(engines, [(0, utts[0], utts[0].n_in(2))]))
        for s in range(3):
            eng.stream_slot_reset(s)
        batched(engines, [(s, v, v.n_in(1)) for s, v in enumerate(utts)])
        three = profiled(lambda: batched(engines, [(s, v, v.n_in(2)) for s, v in enumerate(utts)]))
        assert [eng.stream_slot_rows(s) for s in range(3)] == [v.rows(v.n_in(2)) for v in utts]
    finally:
        eng.close_streams()
    steps, depth = cfg.n_timesteps, cfg.depth
    n1, n3 = {k: v[1] for k, v in one.items()}, {k: v[1] for k, v in three.items()}
    # per step: the input projection, four products per block, the output projection on the register-staged kernel (one launch per
    # weight plane; the synthetic weights have one)
    assert n1["gemm_split"] == steps * (4 * depth + 2) and n1["dit_attention_split"] == steps * depth and n1["conv_mfma"] >= 2 * steps, n1
    assert n1["gemm_bf16"] == 0 and n1["dit_attention"] == 0, n1
    assert n3 == n1, (n3, n1)


def test_errors_and_lifecycle(engines):
    cfg, eng, ref, noise, _ = engines
    X, Y = Utt("a", 50, cfg), Utt("b", 40, cfg)
    before = ref.inference(*X.args(X.n_in(2), noise), flags=FY_PRECISE)       # a precise whole-sequence call, no session yet
    want = eng.inference(*X.args(X.n_in(2), noise), flags=FY_PRECISE)
    assert torch.equal(want, before)
    eng.open_streams(2, CAP, precise=True)
    try:
        b0 = eng.streams_bytes
        assert b0 > 0
        eng.stream_slot_reset(0)
        eng.stream_slot_reset(1)
        poll(engines, [(0, X, X.n_in(1))], flags=0)
        assert eng.streams_bytes == b0                                           # the default mode needs no lo planes
        poll(engines, [(1, Y, Y.n_in(1))])
        b1 = eng.streams_bytes
        R, inner = 2 * 2 * CAP, cfg.heads * cfg.head_dim
        lo = 2 * R * (cfg.n_timesteps * cfg.depth * 3 * inner + 4 * cfg.mel + cfg.dim + inner + cfg.dim * cfg.ff_mult)
        assert b1 == b0 + lo, (b0, b1, lo)                                       # the caches a second time + the work buffers' lo planes
        poll(engines, [(1, Y, Y.n_in(2))])
        assert eng.streams_bytes == b1
        keep = [eng.stream_slot_rows(0), eng.stream_slot_rows(1)]
        for flags in (FY_DIRECT, FY_PRECISE | FY_DIRECT):
            with pytest.raises(_lib.FyError, match=r"error -1:.*FY_DIRECT"):
                batched(engines, [(0, X, X.n_in(2)), (1, Y, Y.n_in(3))], flags)
        with pytest.raises(_lib.FyError, match=r"error -1:"):
            batched(engines, [(1, Y, Y.n_in(3)), (1, X, X.n_in(1))])             # a slot twice: checked before anything moves
        assert [eng.stream_slot_rows(0), eng.stream_slot_rows(1)] == keep == [X.rows(X.n_in(1)), Y.rows(Y.n_in(2))]
        poll(engines, [(1, Y, Y.n_in(3)), (0, X, X.n_in(2))], flags=0, keeps=[Y.rows(Y.n_in(3)), X.rows(X.n_in(2))])
        # the whole-sequence precise call on the same handle, beside the open session
        assert torch.equal(eng.inference(*X.args(X.n_in(2), noise), flags=FY_PRECISE), want)
        # a session opened without precise=True takes the default arithmetic only, as before: the flag is refused, nothing moves
        eng.open_streams(2, CAP)
        assert eng.streams_bytes == b0
        eng.stream_slot_reset(0)
        poll(engines, [(0, X, X.n_in(1))], flags=0)
        with pytest.raises(_lib.FyError, match=r"error -1:.*FY_PRECISE"):
            batched(engines, [(0, X, X.n_in(2))])
        assert eng.stream_slot_rows(0) == X.rows(X.n_in(1)) and eng.streams_bytes == b0
        poll(engines, [(0, X, X.n_in(2))], flags=0)
    finally:
        eng.close_streams()
    assert eng.streams_bytes == 0
    assert torch.equal(eng.inference(*X.args(X.n_in(2), noise), flags=FY_PRECISE), want)
    with pytest.raises(_lib.FyError, match=r"error -4:"):
        batched(engines, [(0, X, X.n_in(1))])                                    # no session


def test_general_fp32_weights():
    """A general fp32 checkpoint (fy_flow_weight_planes == 2: both weight planes in every split product, the position convs on
    the exact fp32 kernel), state dict built as tests/test_fp32w_gpu.py builds it.  Full size: two streams, two polls, equal to
    the solo precise recompute.  The comparison with the CPU oracle's streaming path (oracle.flow.inference(streaming=True,
    finalize=False)), held to the mode's bar rtol 1e-2 / atol 1e-4 (cosyvoice/bin/export_onnx.py:109), runs at the REDUCED-size
    config FlowCfg.tiny(): the full-size oracle is ~0.7 TFLOP on the CPU for one 100-row chunk, far beyond a few seconds."""
    from fangyan_tts_amd.flow import FlowEngine
    from oracle import flow as oflow
    cfg = FlowCfg()
    with synth.unrounded_weights():
        sd = synth.state_dict_torch(cfg.manifest(), DEV)
    E = make_engines(cfg, sd)
    eng, ref = E[1], E[2]
    try:
        assert eng.weight_planes == 2 and ref.weight_planes == 2
        utts = [Utt("g", 25, cfg), Utt("h", 13, cfg)]
        eng.open_streams(2, CAP, precise=True)
        for k in range(1, 3):
            poll(E, [(s, u, u.n_in(k)) for s, u in enumerate(utts)])
    finally:
        eng.close()
        ref.close()
    tiny = FlowCfg.tiny()
    with synth.unrounded_weights():
        sd_np = synth.state_dict(tiny.manifest())
    sd = {k: torch.from_numpy(v).to(DEV) for k, v in sd_np.items()}
    te = FlowEngine(sd, tiny, max_batch=1, max_frames=CAP, device=DEV)
    try:
        assert te.weight_planes == 2
        P = oflow.prepare(sd_np)
        noise = torch.from_numpy(synth.flow_rand_noise(CAP))
        utts = [Utt("tg", 25, tiny), Utt("th", 13, tiny)]
        Et = (tiny, te, None, noise, {})
        te.open_streams(2, CAP, precise=True)
        batched(Et, [(s, u, u.n_in(1)) for s, u in enumerate(utts)])
        mel = batched(Et, [(s, u, u.n_in(2)) for s, u in enumerate(utts)]).cpu()
        u = utts[1]
        n_in = u.n_in(2)
        want = oflow.inference(u.token[:, :n_in], u.ptoken, u.pfeat, u.emb, P, tiny, noise.reshape(1, tiny.mel, -1), streaming=True, finalize=False)
        got = mel[1:2, :, :2 * (n_in - LOOK)]
        assert got.shape == want.shape
        err = (got - want).abs()
        print("precise slots vs oracle, reduced size: max |err| %.3e" % float(err.max()))
        assert bool((err <= 1e-4 + 1e-2 * want.abs()).all()), float(err.max())
    finally:
        te.close()


def test_facade_precise_streams():
    """Reduced-size model with flow_flags = FY_PRECISE: the chunks of tts(stream=True) are the same tensors with and without
    incremental_stream, and tts_stream_batch over 3 utterances yields, per stream, the chunks tts(stream=True) yields for it alone."""
    from fangyan_tts_amd.cli.model import CosyVoice3Model
    cfg = ModelCfg.tiny()
    cases = [(40, 6, 0, 12), (30, 5, 0, 25), (24, 4, 0, 7)]
    sd = [synth.state_dict_torch(m.manifest(), DEV, skip=("lm_head",)) for m in (cfg.llm, cfg.flow, cfg.hift)]
    n_text_max = max(c[0] for c in cases)
    m = CosyVoice3Model(sd[0], sd[1], sd[2], cfg, device=DEV, max_batch=len(cases), max_text=64, max_prompt_tokens=32, max_tokens=20 * n_text_max,
                        rand_noise=torch.from_numpy(synth.flow_rand_noise(2 * (32 + 20 * n_text_max))),
                        rand_ini=torch.from_numpy(synth.hift_rand_ini()), sine_noise=torch.from_numpy(synth.hift_sine_noise(2 * 20 * n_text_max * 480)))
    m.flow_flags = FY_PRECISE
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
    assert m.incremental_stream
    alone = [[o["tts_speech"] for o in m.tts(**inp, stream=True)] for inp in inputs]
    assert any(ln.flow.stream_rows() > 0 for ln in m.lanes)              # the precise chunks were incremental
    m.incremental_stream = False
    try:
        plain = [o["tts_speech"] for o in m.tts(**inputs[0], stream=True)]
    finally:
        m.incremental_stream = True
    assert len(plain) == len(alone[0]) >= 2
    for k, (x, y) in enumerate(zip(alone[0], plain)):
        assert x.shape == y.shape and torch.equal(x, y), k
    got = [[] for _ in inputs]
    for i, o in m.tts_stream_batch(inputs):
        got[i].append(o["tts_speech"])
    for i in range(len(inputs)):
        assert len(got[i]) == len(alone[i]) >= 2, i
        for k, (x, y) in enumerate(zip(got[i], alone[i])):
            assert x.device.type == "cpu" and x.shape == y.shape and torch.equal(x, y), (i, k)
    assert all(ln.flow.streams_bytes == 0 for ln in m.lanes)
