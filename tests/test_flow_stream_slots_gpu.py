"""Flow stream slots (csrc/flow.hip: fy_flow_infer_streams): several stream=True utterances advance by a chunk each in ONE pass.

The contract is the single stream's (tests/test_stream_gpu.py::test_flow_incremental_chunks_equal_full_recompute): every chunk of
every stream equals, BIT FOR BIT over its valid frames, the full recompute of that stream alone - `inference(..., streaming=True,
finalize=False)` at B = 1 on a second engine, the non-incremental path.  No tolerance anywhere: rows of a product do not depend on
the tile they sit in, LayerNorm-modulate and the convolutions are per row, attention is per query.  Full-size FlowCfg(), synthetic
weights.  The reference's chunk schedule: 25-token hops, 3 look-ahead tokens, the first hop padded so that prompt + hop is a
multiple of 25 tokens.
"""
import pytest
import torch

from fangyan_tts_amd import _lib, synth
from fangyan_tts_amd.spec import FlowCfg
from gpu_util import maxerr, synth_mel

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HOP, LOOK = 25, 3
K_MAX, P_MAX = 5, 75
N_MAX = K_MAX * HOP + 24 + LOOK + 4                       # tokens of the longest call (the largest first-hop pad, an off-boundary tail)
CAP = 2 * (N_MAX + P_MAX)


class Utt:
    """One utterance's inputs; n_in(k) = tokens of its k-th chunk call (k = 1, 2, ...)."""

    def __init__(self, tag, p_tok, cfg):
        self.p_tok = p_tok
        self.token = torch.from_numpy(synth.randint(f"in.flow.token.slots.{tag}", (1, N_MAX), 0, cfg.vocab))
        self.ptoken = torch.from_numpy(synth.randint(f"in.flow.ptoken.slots.{tag}", (1, max(p_tok, 1)), 0, cfg.vocab))[:, :p_tok]
        self.pfeat = torch.from_numpy(synth_mel(f"in.flow.pfeat.slots.{tag}", 2 * max(p_tok, 1)))[:, :2 * p_tok]
        self.emb = torch.from_numpy(synth.normal(f"in.flow.spk.slots.{tag}", (1, cfg.spk_in)))
        self.pad = -(-p_tok // HOP) * HOP - p_tok

    def n_in(self, k):
        return k * HOP + self.pad + LOOK

    def rows(self, n_in):
        return 2 * (self.p_tok + n_in - LOOK)


@pytest.fixture(scope="module")
def engines():
    from fangyan_tts_amd.flow import FlowEngine
    cfg = FlowCfg()
    sd = synth.state_dict_torch(cfg.manifest(), DEV)
    eng = FlowEngine(sd, cfg, max_batch=1, max_frames=CAP, device=DEV)
    ref = FlowEngine(sd, cfg, max_batch=1, max_frames=CAP, device=DEV)
    noise = torch.from_numpy(synth.flow_rand_noise(CAP))
    return cfg, eng, ref, noise


def full(ref, noise, u, n_in):
    return ref.inference(u.token[:, :n_in].contiguous(), [n_in], u.ptoken, [u.p_tok], u.pfeat, [2 * u.p_tok], u.emb, noise,
                         streaming=True, finalize=False)


def batched(eng, noise, calls, flags=0):
    """calls: [(slot, Utt, n_in)] -> mel (n, 80, frames) of one inference_streams call."""
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


def poll(eng, ref, noise, calls, keeps=None):
    """One batched call; every listed stream against its own full recompute, then the rows each slot keeps."""
    mel = batched(eng, noise, calls)
    for i, (slot, u, n_in) in enumerate(calls):
        valid = 2 * (n_in - LOOK)
        want = full(ref, noise, u, n_in)
        assert torch.equal(mel[i, :, :valid], want[0, :, :valid]), (slot, n_in, maxerr(mel[i, :, :valid], want[0, :, :valid]))
        keep = u.rows(n_in) if keeps is None else keeps[i]
        assert eng.stream_slot_rows(slot) == keep, (slot, n_in)


def test_ragged_streams_equal_full_recompute(engines):
    cfg, eng, ref, noise = engines
    utts = [Utt("a", 50, cfg), Utt("b", 40, cfg), Utt("c", 75, cfg), Utt("d", 13, cfg)]      # 40 and 13: padded first hops
    eng.open_streams(4, CAP)
    try:
        assert eng.streams_bytes > 0
        for s in range(4):
            eng.stream_slot_reset(s)
        for k in range(1, 5):
            poll(eng, ref, noise, [(s, u, u.n_in(k)) for s, u in enumerate(utts)])
    finally:
        eng.close_streams()
    assert eng.streams_bytes == 0


def test_staggered_streams(engines):
    cfg, eng, ref, noise = engines
    A, B, C_, D = Utt("sa", 50, cfg), Utt("sb", 40, cfg), Utt("sc", 25, cfg), Utt("sd", 62, cfg)
    eng.open_streams(3, CAP)
    try:
        eng.stream_slot_reset(0)
        poll(eng, ref, noise, [(0, A, A.n_in(1))])
        poll(eng, ref, noise, [(0, A, A.n_in(2))])
        eng.stream_slot_reset(1)                                                  # B joins while A is at chunk 3
        poll(eng, ref, noise, [(0, A, A.n_in(3)), (1, B, B.n_in(1))])
        poll(eng, ref, noise, [(1, B, B.n_in(2))])                                # A sits this poll out ...
        assert eng.stream_slot_rows(0) == A.rows(A.n_in(3))
        eng.stream_slot_reset(2)
        poll(eng, ref, noise, [(2, C_, C_.n_in(1)), (0, A, A.n_in(4)), (1, B, B.n_in(3))])      # ... and continues
        eng.stream_slot_reset(0)                                                  # A has ended: D takes its slot, the neighbours go on
        assert eng.stream_slot_rows(0) == 0
        poll(eng, ref, noise, [(0, D, D.n_in(1)), (1, B, B.n_in(4)), (2, C_, C_.n_in(2))])
        poll(eng, ref, noise, [(2, C_, C_.n_in(3)), (0, D, D.n_in(2))])
    finally:
        eng.close_streams()


def test_fallbacks_and_errors(engines):
    cfg, eng, ref, noise = engines
    X, Y, Z = Utt("fx", 50, cfg), Utt("fy", 40, cfg), Utt("fz", 25, cfg)
    eng.open_streams(2, CAP)
    try:
        eng.stream_slot_reset(0)
        eng.stream_slot_reset(1)
        poll(eng, ref, noise, [(0, X, X.n_in(1)), (1, Y, Y.n_in(1))])
        # X ends off the mask boundary: computed in full, keeps nothing; Y beside it stays incremental
        off = X.n_in(2) + 4
        poll(eng, ref, noise, [(0, X, off), (1, Y, Y.n_in(2))], keeps=[0, Y.rows(Y.n_in(2))])
        poll(eng, ref, noise, [(0, X, X.n_in(3)), (1, Y, Y.n_in(3))])
        # a caller that forgets the reset: another prompt length, or fewer tokens than the slot holds, starts the slot over
        poll(eng, ref, noise, [(1, Z, Z.n_in(2)), (0, X, X.n_in(4))])
        poll(eng, ref, noise, [(1, Z, Z.n_in(3))])
        poll(eng, ref, noise, [(1, Z, Z.n_in(1))])
        keep = [eng.stream_slot_rows(0), eng.stream_slot_rows(1)]
        for calls, flags in (([(0, X, X.n_in(1)), (0, Y, Y.n_in(1))], 0),                  # a slot twice
                             ([(2, X, X.n_in(1))], 0), ([(-1, X, X.n_in(1))], 0),           # outside the session
                             ([(0, X, X.n_in(1))], _lib.FY_PRECISE), ([(0, X, X.n_in(1))], _lib.FY_DIRECT)):
            with pytest.raises(_lib.FyError, match=r"error -1:"):
                batched(eng, noise, calls, flags)
        assert [eng.stream_slot_rows(0), eng.stream_slot_rows(1)] == keep == [X.rows(X.n_in(4)), Z.rows(Z.n_in(1))]      # the session is as it was
        eng.open_streams(2, 2 * (X.p_tok + X.n_in(1) - LOOK))                               # room for X's first chunk only
        batched(eng, noise, [(0, X, X.n_in(1))])
        with pytest.raises(_lib.FyError, match=r"error -1:"):
            batched(eng, noise, [(0, X, X.n_in(2))])                                        # T above cap_frames
        # the caches do not fit: the status says so, nothing is launched, nothing smaller is opened in their place
        with pytest.raises(_lib.FyError, match=r"error -2:.*bytes"):
            eng.open_streams(8, 1 << 28)
    finally:
        eng.close_streams()
    with pytest.raises(_lib.FyError, match=r"error -4:"):
        batched(eng, noise, [(0, X, X.n_in(1))])                                            # no session


def _launches(fn, names=("gemm_bf16", "dit_attention", "conv_mfma")):
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


def test_one_launch_chain_per_poll(engines):
    """A call that advances K = 4 streams by a chunk each issues the DiT products, the attention and the position convs of ONE
    single-stream incremental call - not K times as many."""
    cfg, eng, ref, noise = engines
    utts = [Utt("a", 50, cfg), Utt("b", 40, cfg), Utt("c", 75, cfg), Utt("d", 13, cfg)]
    u = utts[0]
    eng.stream_reset()
    args = lambda n_in: (u.token[:, :n_in].contiguous(), [n_in], u.ptoken, [u.p_tok], u.pfeat, [2 * u.p_tok], u.emb, noise)
    eng.inference(*args(u.n_in(1)), streaming=True, finalize=False, incremental=True)
    one = _launches(lambda: eng.inference(*args(u.n_in(2)), streaming=True, finalize=False, incremental=True))
    assert eng.stream_rows() == u.rows(u.n_in(2))
    eng.open_streams(4, CAP)
    try:
        batched(eng, noise, [(s, v, v.n_in(1)) for s, v in enumerate(utts)])
        four = _launches(lambda: batched(eng, noise, [(s, v, v.n_in(2)) for s, v in enumerate(utts)]))
        assert [eng.stream_slot_rows(s) for s in range(4)] == [v.rows(v.n_in(2)) for v in utts]
    finally:
        eng.close_streams()
    steps, depth = cfg.n_timesteps, cfg.depth
    assert one["gemm_bf16"] == steps * (4 * depth + 2) and one["dit_attention"] == steps * depth and one["conv_mfma"] >= 2 * steps, one
    assert four == one, (four, one)


def test_single_stream_api_untouched(engines):
    """The single stream's sequence gives the same results on a handle that opens, uses and closes a slot session in between."""
    cfg, eng, ref, noise = engines
    u, w = Utt("a", 50, cfg), Utt("b", 40, cfg)
    eng.stream_reset()
    for k in range(1, 5):
        n_in = u.n_in(k)
        args = (u.token[:, :n_in].contiguous(), [n_in], u.ptoken, [u.p_tok], u.pfeat, [2 * u.p_tok], u.emb, noise)
        want = ref.inference(*args, streaming=True, finalize=False)
        inc = eng.inference(*args, streaming=True, finalize=False, incremental=True)
        valid = 2 * (n_in - LOOK)
        assert torch.equal(inc[:, :, :valid], want[:, :, :valid]), k
        assert eng.stream_rows() == u.rows(n_in)
        if k == 2:
            eng.open_streams(2, CAP)
            poll(eng, ref, noise, [(1, w, w.n_in(1)), (0, u, u.n_in(1))])
            poll(eng, ref, noise, [(0, u, u.n_in(2)), (1, w, w.n_in(2))])
            eng.close_streams()
            assert eng.stream_rows() == u.rows(n_in)
