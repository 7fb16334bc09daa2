"""GPU parity of the LM's decode slots (fy_llm_slots_open / fy_llm_slot_join / fy_llm_slot_release): sequences that join and
leave the batch between token steps emit the ids they emit alone.

Yardsticks, in order of authority: the reference-minted fixtures (llm_tiny / llm_full / llm_*_fp32w / llm_ras_tiny); where the
fixtures hold no such case, oracle.llm on the CPU at the reduced size.  Ids compare with ==; there is no tolerance in this file.
"""
from collections import deque

import numpy as np
import pytest
import torch

from _digest import check
from fangyan_tts_amd import synth
from fangyan_tts_amd._lib import FyError
from fangyan_tts_amd.llm import plan_slots
from fangyan_tts_amd.spec import LlmCfg
from gpu_util import golden, llm_case, note

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ERR_ARG, ERR_STATE = "error -1:", "error -4:"


def make(cfg, max_batch=4, max_ctx=512, unrounded=False):
    from fangyan_tts_amd.llm import LlmEngine
    if unrounded:
        with synth.unrounded_weights():
            sd = synth.state_dict_torch(cfg.manifest(), DEV, skip=("lm_head",))
    else:
        sd = synth.state_dict_torch(cfg.manifest(), DEV, skip=("lm_head",))
    return LlmEngine(sd, cfg, max_batch=max_batch, max_ctx=max_ctx, weight_planes=0)


@pytest.fixture(scope="module")
def tiny():
    eng = make(LlmCfg.tiny())
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def full():
    eng = make(LlmCfg(), max_batch=4, max_ctx=256)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def oracle_tiny():
    cfg = LlmCfg.tiny()
    sd = synth.state_dict_torch(cfg.manifest(), torch.device("cpu"), skip=("lm_head",))
    return {k: v.cpu() for k, v in sd.items()}


def oracle_ids(P, cfg, t, pt, pk, n):
    """oracle.llm.inference under the forced length n (min_len = max_len = n), silent-token filter applied"""
    from oracle import llm as ollm
    ref = list(ollm.inference(torch.tensor([t]), torch.tensor([pt]), torch.tensor([pk], dtype=torch.long).reshape(1, -1), P, cfg, min_len=n, max_len=n))
    assert len(ref) == n
    return ollm.silent_filter(ref)


def case(cfg, c):
    return llm_case(cfg, *c, "%d_%d_%d" % c)


def join1(eng, slot, inputs, **kw):
    t, pt, pk = inputs
    eng.join([slot], [t], [pt], [pk], **kw)


def drain(eng, piece=8):
    n, fin, k = None, [False], 0
    while not all(fin):
        n, fin = eng.step(piece)
        k += 1
        assert k < 400
    return n


def ras_rows(rows, n_rows):
    """uniforms (n_rows, 4096): row `slot` = the stream the fixture mint drew for `case`; rows: {slot: case}"""
    u = np.zeros((n_rows, 4096), dtype=np.float32)
    for slot, c in rows.items():
        u[slot] = synth.uniform("in.llm.ras_u.%d_%d_%d" % c, (4096,), 0.0, 1.0)
    return torch.from_numpy(u).to(DEV)


def set_mode(eng, mode):
    eng.set_sampler("greedy")
    eng.set_decode_mode(mode)
    assert eng.decode_mode == mode, "every decode path must be available for the test architectures"


def staggered(eng, f, cases, cap):
    """case 0 into slot 2, five token steps, case 1 into slot 0, to the end -> both id lists equal the fixture's"""
    cfg = eng.cfg
    ins = [case(cfg, c) for c in cases]
    mx = [cap if cap else 20 * len(i[0]) for i in ins]
    out, _, _ = eng.open_slots(max(mx))
    join1(eng, 2, ins[0], max_len=[mx[0]])
    assert eng.live() == [2]
    n, fin = eng.step(5)
    assert n[2] == 6 and not fin[2] and fin[0] and fin[1] and fin[3] and n[0] == 0
    join1(eng, 0, ins[1], max_len=[mx[1]])
    assert eng.live() == [0, 2]
    n = drain(eng)
    out = out.cpu()
    for slot, c in ((2, cases[0]), (0, cases[1])):
        ref = f["c%d_%d_%d.tokens" % c].tolist()
        ref = ref[:cap] if cap else ref
        got = out[slot, : n[slot]].tolist()
        first_bad = next((i for i, (g, r) in enumerate(zip(got, ref)) if g != r), None)
        assert got == ref, (c, slot, first_bad, len(got), len(ref))


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_staggered_joins_tiny(tiny, mode):
    set_mode(tiny, mode)
    staggered(tiny, golden("llm_tiny.npz"), [(12, 8, 0), (10, 6, 30)], None)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_staggered_joins_full(full, mode):
    set_mode(full, mode)
    staggered(full, golden("llm_full.npz"), [(12, 8, 0), (14, 10, 40)], 60)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("size", ["tiny", "full"])
def test_staggered_joins_two_weight_planes(size, mode):
    """Handles built from the unrounded weights store two planes per matrix; the paths that mode has are one launch per
    operation (0) and the few-CU persistent step (1: the 8-row persistent step keeps one plane only)."""
    cfg = LlmCfg.tiny() if size == "tiny" else LlmCfg()
    eng = make(cfg, max_batch=4, max_ctx=512 if size == "tiny" else 256, unrounded=True)
    try:
        assert eng.weight_planes == 2
        set_mode(eng, mode)
        cases, cap = ([(12, 8, 0), (10, 6, 30)], None) if size == "tiny" else ([(12, 8, 0), (14, 10, 40)], 60)
        staggered(eng, golden(f"llm_{size}_fp32w.npz"), cases, cap)
    finally:
        eng.close()


@pytest.mark.parametrize("mode", [1, 0])
def test_crossing_eight_live_slots_both_ways(oracle_tiny, mode):
    """max_batch 32: six sequences, six more after three steps (12 live: the step moves from the 8-row persistent kernel, which
    reads h, to the 32-row forms, which read the A image), the short ones in the high slots end and are released (8 live in
    slots 0 .. 7: back on the 8-row kernel), to the end.  Forced lengths fix the schedule; every id list equals the oracle's."""
    cfg = LlmCfg.tiny()
    eng = make(cfg, max_batch=32, max_ctx=128)
    try:
        set_mode(eng, mode)
        lens = [40, 44, 48, 36, 50, 42, 30, 34, 8, 10, 12, 9]
        ins = [llm_case(cfg, 6 + i % 5, 3 + i % 4, (i % 3) * 4, f"slots.cross.{i}") for i in range(12)]
        out, _, _ = eng.open_slots(64)

        def join(idx):
            eng.join(idx, [ins[i][0] for i in idx], [ins[i][1] for i in idx], [ins[i][2] for i in idx], min_len=[lens[i] for i in idx],
                     max_len=[lens[i] for i in idx])
        join(list(range(6)))
        eng.step(3)
        join(list(range(6, 12)))
        live, got = [len(eng.live())], {}
        k = 0
        while eng.live():
            n, fin = eng.step(4)
            host = out.cpu()
            for s in eng.live():
                if fin[s]:
                    got[s] = host[s, : n[s]].tolist()
                    eng.release(s)
            live.append(len(eng.live()))
            k += 1
            assert k < 100
        note("parity_llm_slots.json", f"crossing.mode{mode}.live_per_poll", live)
        up = next(i for i, v in enumerate(live) if v > 8)
        assert any(0 < v <= 8 for v in live[up + 1:]), live
        for i in range(12):
            assert got[i] == oracle_ids(oracle_tiny, cfg, *ins[i], lens[i]), (i, lens[i])
    finally:
        eng.close()


@pytest.mark.parametrize("kind", ["ras", "greedy"])
def test_release_and_reuse(tiny, kind):
    """A slot released in mid-generation and joined again: the new occupant meets nothing of the old one (position and KV,
    counts, silent run, sampling window, uniforms counter) - its ids are the fixture's, and so are the neighbour's."""
    from oracle.llm import silent_filter
    set_mode(tiny, 1)
    cfg = tiny.cfg
    if kind == "ras":
        f, keep, first, second = golden("llm_ras_tiny.npz"), (12, 8, 0), (30, 5, 0), (16, 4, 10)
        u1, u2 = ras_rows({0: keep, 1: first}, tiny.max_batch), ras_rows({0: keep, 1: second}, tiny.max_batch)
        tiny.set_sampler("ras", u1)
    else:
        f, keep, first, second = golden("llm_tiny.npz"), (12, 8, 0), (12, 8, 0), (10, 6, 30)
    cap = lambda c: [min(20 * c[0], 400)]
    try:
        out, _, _ = tiny.open_slots(400)
        tiny.join([0, 1], *(list(x) for x in zip(case(cfg, keep), case(cfg, first))), max_len=cap(keep) + cap(first))
        n, fin = tiny.step(7)
        assert n[1] >= 1 and not fin[1]
        tiny.release(1)
        assert tiny.live() == [0]
        if kind == "ras":
            tiny.set_sampler("ras", u2)          # row 0 unchanged: slot 0 goes on in its stream; slot 1 reads its row from the start
        join1(tiny, 1, case(cfg, second), max_len=cap(second))
        n = drain(tiny)
        out = out.cpu()
        for slot, c in ((1, second), (0, keep)):
            assert out[slot, : n[slot]].tolist() == silent_filter(f["c%d_%d_%d.tokens" % c].tolist()), (kind, slot, c)
    finally:
        tiny.set_sampler("greedy")


def test_ras_slots_against_reference(tiny):
    """The reference's sampler per slot: the three fixture cases joined at different steps into different slots, each slot's
    uniforms row its case's stream -> ids equal silent_filter(fixture).  Then the give-up case beside a good one: the step
    reports the reference's message with the slot once, and the good sequence's ids still match."""
    from oracle.llm import silent_filter
    f = golden("llm_ras_tiny.npz")
    set_mode(tiny, 1)
    cfg = tiny.cfg
    plan = [(3, (12, 8, 0), 3), (1, (16, 4, 10), 4), (0, (30, 5, 0), 0)]          # slot, case, steps after its join
    try:
        u = ras_rows({s: c for s, c, _ in plan}, tiny.max_batch)
        tiny.set_sampler("ras", u)
        out, _, _ = tiny.open_slots(400)
        for s, c, k in plan:
            join1(tiny, s, case(cfg, c), max_len=[min(20 * c[0], 400)])
            tiny.step(k)
        n = drain(tiny)
        host = out.cpu()
        for s, c, _ in plan:
            assert host[s, : n[s]].tolist() == silent_filter(f["c%d_%d_%d.tokens" % c].tolist()), (s, c)
        bad, good = (10, 6, 30), (12, 8, 0)
        assert "max_trials" in str(f["c%d_%d_%d.raised" % bad])
        u2 = ras_rows({0: good, 2: bad}, tiny.max_batch)
        tiny.set_sampler("ras", u2)
        out, _, _ = tiny.open_slots(400)
        tiny.join([0, 2], *(list(x) for x in zip(case(cfg, good), case(cfg, bad))), max_len=[240, 200])
        raised, fin, k = [], [False], 0
        while not all(fin):
            try:
                n, fin = tiny.step(8)
            except FyError as e:
                raised.append(str(e))
            k += 1
            assert k < 100
        assert len(raised) == 1 and "sampling reaches max_trials 100" in raised[0] and "slot 2" in raised[0] and ERR_STATE in raised[0], raised
        assert out.cpu()[0, : n[0]].tolist() == silent_filter(f["c%d_%d_%d.tokens" % good].tolist())
    finally:
        tiny.set_sampler("greedy")


def test_join_embeds_equals_join(tiny):
    """fy_llm_slot_join_embeds (the add_request shape) against fy_llm_slot_join on the same sequences: the host assembles
    lm_input as tests/test_llm_gpu.py::test_prefill_from_embeddings_equals_begin does, fp32 and bf16 rows -> identical ids, and
    the fixture's for case 0."""
    from oracle.llm import silent_filter
    set_mode(tiny, 1)
    cfg = tiny.cfg
    cases, slots = [(12, 8, 0), (16, 4, 10)], [3, 1]
    texts, ptexts, ptoks = (list(x) for x in zip(*[case(cfg, c) for c in cases]))
    cap = [min(20 * len(t), 400) for t in texts]
    mn = [2 * len(t) for t in texts]
    out, _, _ = tiny.open_slots(400)
    tiny.join(slots, texts, ptexts, ptoks, max_len=cap)
    n0 = drain(tiny)
    whole = out.cpu().clone()
    sd = synth.state_dict_torch(cfg.manifest(), DEV, skip=("lm_head",))
    emb_tok = sd["llm.model.model.embed_tokens.weight"].to(torch.bfloat16).float()       # the engine keeps embed_tokens in bf16
    emb_sp = sd["speech_embedding.weight"]
    for dt in (torch.float32, torch.bfloat16):
        rows = []
        for b in range(len(cases)):
            ids = torch.tensor(list(ptexts[b]) + list(texts[b]), dtype=torch.long, device=DEV)
            parts = [emb_sp[cfg.speech_tokens: cfg.speech_tokens + 1], emb_tok[ids], emb_sp[cfg.speech_tokens + 2: cfg.speech_tokens + 3]]
            if len(ptoks[b]):
                parts.append(emb_sp[torch.tensor(list(ptoks[b]), dtype=torch.long, device=DEV)])
            rows.append(torch.cat(parts, dim=0).to(dt))
        out, _, _ = tiny.open_slots(400)
        tiny.join_embeds(slots[:1], rows[:1], mn[:1], cap[:1])
        tiny.step(3)
        tiny.join_embeds(slots[1:], rows[1:], mn[1:], cap[1:])
        n = drain(tiny)
        assert n == n0, (dt, n, n0)
        host = out.cpu()
        for s in slots:
            assert host[s, : n[s]].tolist() == whole[s, : n[s]].tolist(), (dt, s)
    f = golden("llm_tiny.npz")
    assert whole[slots[0], : n0[slots[0]]].tolist() == silent_filter(f["c%d_%d_%d.tokens" % cases[0]].tolist())


def test_generate_continuous_follows_the_plan(oracle_tiny):
    """40 requests of ragged forced lengths through 8 slots: every id list equals the oracle's for that request alone, and the
    token steps the library launched are plan_slots'."""
    cfg = LlmCfg.tiny()
    eng = make(cfg, max_batch=8, max_ctx=96)
    try:
        set_mode(eng, 1)
        N = 40
        lens = synth.randint("slots.gc.len", (N,), 3, 41).tolist()
        ins = [llm_case(cfg, 6 + i % 7, 3 + i % 4, (i % 3) * 5, f"slots.gc.{i}") for i in range(N)]
        texts, ptexts, ptoks = (list(x) for x in zip(*ins))
        ids, raw = eng.generate_continuous(texts, ptexts, ptoks, min_len=lens, max_len=lens, steps_per_poll=8)
        steps, joins = plan_slots(lens, 8, 8)
        note("parity_llm_slots.json", "generate_continuous.steps", [eng.slot_steps, steps, len(joins)])
        assert raw == lens
        assert eng.slot_steps == steps
        assert eng.live() == []
        for i in range(N):
            assert ids[i] == oracle_ids(oracle_tiny, cfg, *ins[i], lens[i]), (i, lens[i])
    finally:
        eng.close()


def test_errors_leave_the_session_usable(tiny):
    """Every refusal comes before any device work: the sequence running in slot 0 ends with the fixture's ids after all of them.
    (More prefill rows than the workspace cannot be reached through a join whose sequences each fit max_ctx: the workspace holds
    max_batch x max_ctx rows.  The check stands for handles whose limits change.)"""
    f = golden("llm_tiny.npz")
    set_mode(tiny, 1)
    cfg = tiny.cfg
    a, b = case(cfg, (12, 8, 0)), case(cfg, (10, 6, 30))
    tiny.generate([b[0]], [b[1]], [b[2]], max_len=[8])                # no session open (a generate closes one)
    with pytest.raises(FyError, match="no slot session") as e:
        join1(tiny, 0, a)
    assert ERR_STATE in str(e.value)
    with pytest.raises(FyError, match="no slot session"):
        tiny.release(0)
    out, _, _ = tiny.open_slots(400)
    join1(tiny, 0, a)
    tiny.step(4)
    for slots, kw, code, msg in (([tiny.max_batch], {}, ERR_ARG, "outside"), ([-1], {}, ERR_ARG, "outside"), ([0], {}, ERR_STATE, "is live"),
                                 ([1, 1], {}, ERR_ARG, "twice"), ([1], {"max_len": [tiny.max_ctx]}, ERR_ARG, "positions"),
                                 ([1], {"max_len": [0]}, ERR_ARG, "bad lengths")):
        k = len(slots)
        with pytest.raises(FyError, match=msg) as e:
            tiny.join(slots, [b[0]] * k, [b[1]] * k, [b[2]] * k, **({key: v * k for key, v in kw.items()}))
        assert code in str(e.value), (slots, str(e.value))
        assert tiny.live() == [0]
    rows = torch.zeros(4, cfg.hidden, device=DEV)
    with pytest.raises(FyError, match="is live"):
        tiny.join_embeds([0], [rows], [0], [8])
    with pytest.raises(FyError, match="positions"):
        tiny.join_embeds([1], [rows], [0], [tiny.max_ctx])
    with pytest.raises(FyError, match="is free") as e:
        tiny.release(2)
    assert ERR_STATE in str(e.value)
    with pytest.raises(FyError, match="slot session") as e:
        tiny.logp(0, 1)
    assert ERR_STATE in str(e.value)
    n = drain(tiny)
    assert out.cpu()[0, : n[0]].tolist() == f["c12_8_0.tokens"].tolist()
    tiny.release(0)
    assert tiny.live() == []
    n, fin = tiny.step(8)                                             # no live slot: nothing to launch
    assert n == [0] * tiny.max_batch and all(fin) and tiny.slot_steps == 4 + 8 * ((len(f["c12_8_0.tokens"]) - 5 + 8) // 8)


def test_generate_after_a_session_is_unchanged(tiny):
    """fy_llm_generate closes the session and behaves as before it: ids and the kept log-probabilities of llm_tiny.npz."""
    f = golden("llm_tiny.npz")
    set_mode(tiny, 1)
    cfg = tiny.cfg
    cases = [(12, 8, 0), (10, 6, 30)]
    tiny.set_sampler("ras", ras_rows({1: (16, 4, 10), 2: (12, 8, 0)}, tiny.max_batch))
    try:
        tiny.open_slots(400)
        join1(tiny, 2, case(cfg, cases[0]))
        tiny.step(9)
        join1(tiny, 1, case(cfg, (16, 4, 10)))
        tiny.step(5)                                                  # left unfinished on purpose
    finally:
        tiny.set_sampler("greedy")
    texts, ptexts, ptoks = (list(x) for x in zip(*[case(cfg, c) for c in cases]))
    out, out_n, _ = tiny.generate(texts, ptexts, ptoks)
    out, out_n = out.cpu(), out_n.cpu().tolist()
    for b, c in enumerate(cases):
        assert out[b, : out_n[b]].tolist() == f["c%d_%d_%d.tokens" % c].tolist(), c
        for s in range(3):
            check(tiny.logp(s, len(cases))[b].cpu(), f, "c%d_%d_%d.logp%d" % (*c, s), 1e-3, 2e-3)
    with pytest.raises(FyError, match="no slot session"):
        tiny.release(0)
