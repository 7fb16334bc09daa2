"""The non-stream serving loop (CosyVoice3Model.tts_serve) and its device hand-off (fy_llm_slots_export / LlmEngine.export).

Yardsticks: the ids of `tts_batch([request])` and the samples of `tts(**request)` for each request alone (greedy sampling), the
padded flow call + vocoder on a group's own tokens for ragged groups, and `plan_serve` for the schedule.  Ids and samples compare
with == / torch.equal: there is no tolerance in this file."""
import pytest
import torch

from fangyan_tts_amd import synth
from fangyan_tts_amd._lib import FyError
from fangyan_tts_amd.llm import plan_serve
from fangyan_tts_amd.spec import LlmCfg, ModelCfg
from gpu_util import llm_case, synth_mel

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ERR_ARG, ERR_STATE = "error -1:", "error -4:"
# (text ids, prompt-text ids, LM prompt speech tokens, flow prompt tokens) per request; slots per model
CASES = {"tiny": ([(40, 6, 0, 12), (30, 5, 0, 25), (24, 4, 10, 7), (12, 3, 0, 12), (36, 5, 6, 25)], 3),
         "full": ([(8, 8, 0, 25), (6, 5, 0, 12), (7, 4, 5, 30)], 2)}
_worlds = {}


class World:
    """One model per configuration for the whole module, its requests and what each request gives alone."""

    def __init__(self, tag):
        from fangyan_tts_amd.cli.model import CosyVoice3Model
        cases, slots = CASES[tag]
        cfg = ModelCfg.tiny() if tag == "tiny" else ModelCfg()
        sd = [synth.state_dict_torch(m.manifest(), DEV, skip=("lm_head",)) for m in (cfg.llm, cfg.flow, cfg.hift)]
        n_text_max = max(c[0] for c in cases)
        # flow_group=2: the flow decoder and vocoder take 2 x max_batch rows, so a group of 3 fits behind the full model's 2 slots
        self.m = CosyVoice3Model(sd[0], sd[1], sd[2], cfg, device=DEV, max_batch=slots, flow_group=2, max_text=64, max_prompt_tokens=32,
                                 max_tokens=20 * n_text_max, rand_noise=torch.from_numpy(synth.flow_rand_noise(2 * (32 + 20 * n_text_max))),
                                 rand_ini=torch.from_numpy(synth.hift_rand_ini()),
                                 sine_noise=torch.from_numpy(synth.hift_sine_noise(2 * 20 * n_text_max * 480)))
        self.inputs = []
        for n_text, n_ptext, p_llm, p_flow in cases:
            t, pt, pk = llm_case(cfg.llm, n_text, n_ptext, p_llm, f"serve.{n_text}_{n_ptext}_{p_llm}_{p_flow}")
            self.inputs.append({
                "text": torch.tensor([t], dtype=torch.int32), "prompt_text": torch.tensor([pt], dtype=torch.int32),
                "llm_prompt_speech_token": torch.tensor([pk], dtype=torch.int32).reshape(1, -1),
                "flow_prompt_speech_token": torch.from_numpy(synth.randint(f"in.flow.ptoken.serve.{p_flow}", (1, p_flow), 0, 6561)),
                "prompt_speech_feat": torch.from_numpy(synth_mel(f"in.flow.pfeat.serve.{p_flow}", 2 * p_flow)),
                "flow_embedding": torch.from_numpy(synth.normal(f"in.flow.spk.serve.{p_flow}", (1, 192))),
            })
        self.slots = slots
        self.ids = [self.m.tts_batch([inp])[2][0].cpu().tolist() for inp in self.inputs]
        self.speech = [next(self.m.tts(**inp))["tts_speech"] for inp in self.inputs]
        # token steps a request takes in a slot, in plan_serve's terms (the join emits the first token, n - 1 steps follow): its raw
        # count when max_len ended it, one more when a stop token did (the step that samples the stop token emits nothing)
        self.plan_n = []
        for inp in self.inputs:
            t = inp["text"].reshape(-1).tolist()
            _, _, raw = self.m.llm.generate([t], [inp["prompt_text"].reshape(-1).tolist()], [inp["llm_prompt_speech_token"].reshape(-1).tolist()])
            raw = int(raw.cpu()[0])
            self.plan_n.append(raw if raw >= 20 * len(t) else raw + 1)

    def serve(self, requests=None, **kw):
        got = list(self.m.tts_serve(self.inputs if requests is None else requests, record_polls=True, **kw))
        assert sorted(o["index"] for o in got) == list(range(len(self.inputs))), "every index exactly once"
        assert not any("error" in o for o in got)
        return {o["index"]: o for o in got}, got


def world(tag) -> World:
    if tag not in _worlds:
        _worlds[tag] = World(tag)
    return _worlds[tag]


# ---------------------------------------------------------------------------------------------------------------- 1. export
def slot_session(eng, lens, ins):
    out, _, _ = eng.open_slots(64)
    eng.join([0, 1, 2], [i[0] for i in ins], [i[1] for i in ins], [i[2] for i in ins], min_len=lens, max_len=lens)
    eng.step(8)
    n, fin = eng.step(8)
    assert fin == [True, False, True, True] and 1 <= n[0] <= 9 and 1 <= n[1] <= 17 and 1 <= n[2] <= 14 and n[3] == 0
    return out, n


def finish(eng, out, slot):
    fin, k = [False] * 4, 0
    while not fin[slot]:
        n, fin = eng.step(8)
        k += 1
        assert k < 20
    return out.cpu()[slot, : n[slot]].tolist()


def test_export():
    from fangyan_tts_amd.llm import LlmEngine
    cfg = LlmCfg.tiny()
    eng = LlmEngine(synth.state_dict_torch(cfg.manifest(), DEV, skip=("lm_head",)), cfg, max_batch=4, max_ctx=160)
    try:
        lens = [9, 30, 14]                                    # forced lengths (raw counts; the silent-token filter may keep fewer)
        ins = [llm_case(cfg, 8 + 2 * i, 4 + i, 5 * i, f"serve.export.{i}") for i in range(3)]
        out, n = slot_session(eng, lens, ins)
        clean = finish(eng, out, 1)                           # slot 1's ids when nothing else happens

        out, n = slot_session(eng, lens, ins)
        host = out.cpu()
        for order in ([0, 2], [2, 0]):
            for ld in (None, 14, 16, 300):
                tok, counts = eng.export(order, ld)
                width = 64 if ld is None else ld
                assert tok.shape == (2, width) and tok.dtype == torch.int32 and counts == [n[s] for s in order]
                for i, s in enumerate(order):
                    assert tok[i, : n[s]].cpu().tolist() == host[s, : n[s]].tolist(), (order, ld, s)
                    assert int(tok[i, n[s]:].abs().sum()) == 0, (order, ld, s)
        tok, counts = eng.export([1, 2, 0], 10)               # a running slot gives its ids so far; rows longer than ld are cut
        assert counts == [n[1], n[2], n[0]] and max(counts) > 10
        assert tok.cpu().tolist() == [host[s, : min(10, n[s])].tolist() + [0] * (10 - min(10, n[s])) for s in (1, 2, 0)]
        # export, release, a fresh join into the same slot: the exported tensor is not the session's memory
        tok, counts = eng.export([0, 2])
        before = tok.cpu().clone()
        eng.release(0)
        eng.join([0], [ins[2][0]], [ins[2][1]], [ins[2][2]], min_len=[12], max_len=[12])
        n2, _ = eng.step(3)
        torch.cuda.synchronize()
        assert torch.equal(tok.cpu(), before)
        tok2, counts2 = eng.export([0])
        assert counts2 == [n2[0]] and 1 <= n2[0] <= 4 and tok2[0, : n2[0]].cpu().tolist() == out.cpu()[0, : n2[0]].tolist()
        # every refusal comes before any device work
        for slots, ld, code, msg in (([3], None, ERR_STATE, "is free"), ([4], None, ERR_ARG, "outside"), ([-1], None, ERR_ARG, "outside"),
                                     ([1, 1], None, ERR_ARG, "twice"), ([], None, ERR_ARG, r"outside \[1, 4\]"),
                                     ([0, 1, 2, 3, 0], None, ERR_ARG, r"outside \[1, 4\]"), ([1], 0, ERR_ARG, "below 1"), ([1], -3, ERR_ARG, "below 1")):
            with pytest.raises(FyError, match=msg) as e:
                eng.export(slots, ld)
            assert code in str(e.value), (slots, ld, str(e.value))
            assert eng.live() == [0, 1, 2]
        assert finish(eng, out, 1) == clean
        eng.generate([ins[0][0]], [ins[0][1]], [ins[0][2]], max_len=[4])          # closes the session
        with pytest.raises(FyError, match="no slot session") as e:
            eng.export([0], 8)
        assert ERR_STATE in str(e.value)
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------- 2. ids
@pytest.mark.parametrize("tag", ["tiny", "full"])
def test_ids_equal_each_request_alone(tag):
    w = world(tag)
    by, got = w.serve()
    for i in range(len(w.inputs)):
        assert by[i]["tokens"].cpu().tolist() == w.ids[i], i
        assert by[i]["tts_speech"].device.type == "cpu" and by[i]["tts_speech"].shape[0] == 1
    joins = [j for p in w.m.last_serve["polls"] for j in p["joins"]]
    assert len(joins) == len(w.inputs) > w.slots
    if tag == "tiny":                                          # the slots were refilled at least twice
        assert len([p for p in w.m.last_serve["polls"] if p["joins"]]) >= 3
    assert w.m.last_serve["token_steps"] == sum(p["steps"] for p in w.m.last_serve["polls"])
    assert w.m.last_serve["n_joins"] == len(joins) and w.m.last_serve["n_polls"] >= len(w.m.last_serve["polls"])
    assert w.m.last_serve["flow_calls"] == w.m.last_serve["n_groups"] == len({o["group"] for o in got})


# ---------------------------------------------------------------------------------------------------------------- 3. audio, groups of one
@pytest.mark.parametrize("tag", ["tiny", "full"])
def test_audio_group_of_one_equals_tts(tag):
    w = world(tag)
    by, got = w.serve(group_max=1)
    for i in range(len(w.inputs)):
        assert by[i]["group"] == (i,)
        assert by[i]["tts_speech"].shape == w.speech[i].shape, i
        assert torch.equal(by[i]["tts_speech"], w.speech[i]), i


# ---------------------------------------------------------------------------------------------------------------- 4. audio, ragged groups
@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("tag", ["tiny", "full"])
def test_audio_ragged_groups_equal_the_padded_call(tag, packed):
    w = world(tag)
    m, ln = w.m, w.m.lanes[0]
    gmax = 3
    m.flow_packed = packed
    try:
        by, got = w.serve(group_max=gmax, group_wait=10 ** 6)
    finally:
        m.flow_packed = False
    groups = sorted({o["group"] for o in got})
    assert sorted(i for g in groups for i in g) == list(range(len(w.inputs)))
    assert any(len(g) >= 2 and len({len(w.ids[i]) for i in g}) >= 2 for g in groups), groups       # not singletons only
    up = m.cfg.hift.upsample_total
    for g in groups:
        n_tok = [by[i]["tokens"].shape[0] for i in g]
        assert n_tok == sorted(n_tok, reverse=True)
        tok = torch.zeros(len(g), max(n_tok), dtype=torch.int32, device=DEV)
        for j, i in enumerate(g):
            tok[j, : n_tok[j]] = by[i]["tokens"]
        ptok, n_fp, pfeat, n_pf, emb = m._prompt_tensors([w.inputs[i] for i in g])
        mel = ln.flow.inference(tok, n_tok, ptok, n_fp, pfeat, n_pf, emb, m.rand_noise, flags=m.flow_flags, packed=False)
        wav, _ = ln.hift.inference(mel, m.rand_ini, m.sine_noise, frames=[2 * n for n in n_tok], flags=m.hift_flags)
        wav = wav.cpu()
        for j, i in enumerate(g):
            assert by[i]["tts_speech"].shape == (1, 2 * n_tok[j] * up), (g, i)
            assert torch.equal(by[i]["tts_speech"][0], wav[j, : 2 * n_tok[j] * up]), (g, i, packed)


# ---------------------------------------------------------------------------------------------------------------- 5. arrival over time
def test_arrivals_over_time_follow_the_plan():
    w = world("tiny")

    def arriving():
        yield w.inputs[0]
        yield w.inputs[1]
        for _ in range(3):
            yield None
        yield from w.inputs[2:]

    by, got = w.serve(arriving(), steps_per_poll=8, group_max=2, group_wait=1)
    for i in range(len(w.inputs)):
        assert by[i]["tokens"].cpu().tolist() == w.ids[i], i
    # the first None ends poll 0's arrivals, the other two are polls 1 and 2: the late requests arrive in poll 3
    plan = plan_serve(w.plan_n, [0, 0, 3, 3, 3], w.slots, 8, 2, 1, lengths=[len(t) for t in w.ids])
    # the record keeps the polls in which something happened, under their poll numbers
    assert w.m.last_serve["polls"] == [p for p in plan if p["joins"] or p["steps"] or p["retired"] or p["groups"]]
    assert sorted({o["group"] for o in got}) == sorted(g for p in plan for g in p["groups"])


# ---------------------------------------------------------------------------------------------------------------- 6. clean exit
def test_abandoned_generator_leaves_the_model_clean():
    w = world("tiny")
    m, lm = w.m, w.m.lanes[0].llm
    mode = lm.decode_mode
    gen = m.tts_serve(w.inputs, group_max=1)
    first = next(gen)
    assert torch.equal(first["tts_speech"], w.speech[first["index"]])
    gen.close()
    assert lm.decode_mode == mode
    assert m._free.qsize() == len(m.lanes)                    # the lane is back
    assert not any(t.name == "fy-serve-flow" for t in __import__("threading").enumerate())
    assert torch.equal(next(m.tts(**w.inputs[0]))["tts_speech"], w.speech[0])
    lm.open_slots(8)
    assert lm.live() == []


def test_worker_exception_and_capacity_errors_surface():
    """A request over the model's capacity comes back as an error item and the others are served; an exception in the flow
    worker is raised in the consumer, and the model is usable afterwards."""
    w = world("tiny")
    m = w.m
    big = dict(w.inputs[3], text=torch.zeros(1, 65, dtype=torch.int32))                    # max_text is 64
    got = list(m.tts_serve([w.inputs[3], big], group_max=1))
    assert [(o["index"], "error" in o) for o in sorted(got, key=lambda o: o["index"])] == [(0, False), (1, True)]
    assert isinstance(got[0]["error"] if "error" in got[0] else got[1]["error"], ValueError)
    assert torch.equal([o for o in got if o["index"] == 0][0]["tts_speech"], w.speech[3])
    m._token2wav = lambda *a, **k: (_ for _ in ()).throw(RuntimeError("boom in the worker"))
    try:
        with pytest.raises(RuntimeError, match="boom in the worker"):
            list(m.tts_serve([w.inputs[3]]))
    finally:
        del m._token2wav
    assert m._free.qsize() == len(m.lanes)
    assert torch.equal(next(m.tts(**w.inputs[3]))["tts_speech"], w.speech[3])


# ---------------------------------------------------------------------------------------------------------------- idle input
def test_idle_polls_sleep_and_keep_no_record():
    """A generator that has nothing for a while: the idle polls sleep (one host-wait interval each: their number is bounded by the
    time spent, not by how fast the loop can turn), and without record_polls the call keeps counters only."""
    import time
    from fangyan_tts_amd._lib import HOST_WAIT_SLEEP_S
    w = world("tiny")
    t, IDLE_S = {}, 0.02

    def arriving():
        yield w.inputs[3]
        while not t.get("got"):                               # nothing more until the first request has come back
            yield None
        before, end = w.m.last_serve["n_polls"], time.monotonic() + IDLE_S
        while time.monotonic() < end:                         # nothing running, nothing in flight, nothing arriving
            yield None
        t["polls idle"] = w.m.last_serve["n_polls"] - before
        yield w.inputs[2]

    got = []
    for o in w.m.tts_serve(arriving(), group_max=1):
        got.append(o)
        t["got"] = True
    assert [o["index"] for o in got] == [0, 1]
    assert got[0]["tokens"].cpu().tolist() == w.ids[3] and got[1]["tokens"].cpu().tolist() == w.ids[2]
    assert "polls" not in w.m.last_serve and w.m.last_serve["n_joins"] == 2 and w.m.last_serve["n_groups"] == 2
    # every idle poll sleeps at least the interval: no more than IDLE_S / interval of them (a spinning loop makes thousands)
    assert 1 <= t["polls idle"] <= IDLE_S / HOST_WAIT_SLEEP_S + 2, t


# ---------------------------------------------------------------------------------------------------------------- the facade
FACADE_YAML = """
sample_rate: 24000
flow: !new:cosyvoice.flow.flow.CausalMaskedDiffWithDiT
    vocab_size: 6561
    decoder: !new:cosyvoice.flow.flow_matching.CausalConditionalCFM
        cfm_params: !new:omegaconf.DictConfig
            content:
                inference_cfg_rate: 0.7
hift: !new:cosyvoice.hifigan.generator.CausalHiFTGenerator
    upsample_rates: [8, 5, 3]
    nsf_voiced_threshold: 10
"""


class StandInFrontEnd:
    """Deterministic ids / features from the strings (the frontend's ONNX models and tokenizer are not needed for the loop)."""

    def __init__(self, cfg):
        self.cfg, self.spk2info = cfg, {}

    def text_normalize(self, text, split=True, text_frontend=True):
        return [text] if split else text

    def frontend_zero_shot(self, tts_text, prompt_text, prompt_wav, resample_rate, zero_shot_spk_id):
        p = 12
        ids = lambda text, n: torch.from_numpy(synth.randint("serve.fe." + text, (1, n), 0, self.cfg.llm.vocab))
        tok = torch.from_numpy(synth.randint("serve.fe.tok." + prompt_wav, (1, p), 0, 6561))
        emb = torch.from_numpy(synth.normal("serve.fe.spk." + prompt_wav, (1, 192)))
        return {"text": ids(tts_text, 5 + len(tts_text)), "prompt_text": ids(prompt_text, 5), "llm_prompt_speech_token": tok,
                "flow_prompt_speech_token": tok, "prompt_speech_feat": torch.from_numpy(synth_mel("serve.fe.feat." + prompt_wav, 2 * p)),
                "llm_embedding": emb, "flow_embedding": emb}

    def frontend_instruct2(self, tts_text, instruct_text, prompt_wav, resample_rate, zero_shot_spk_id):
        d = self.frontend_zero_shot(tts_text, instruct_text, prompt_wav, resample_rate, zero_shot_spk_id)
        del d["llm_prompt_speech_token"]
        return d

    def frontend_cross_lingual(self, tts_text, prompt_wav, resample_rate, zero_shot_spk_id):
        d = self.frontend_zero_shot(tts_text, "", prompt_wav, resample_rate, zero_shot_spk_id)
        del d["prompt_text"], d["llm_prompt_speech_token"]
        return d


def test_facade_inference_serve(tmp_path):
    """CosyVoice3.inference_serve: (mode, kwargs) items, a None between them, through two slots -> each item's audio is what its
    own inference_* call gives (groups of one), with the item's position attached."""
    from cosyvoice.cli.cosyvoice import AutoModel
    cfg = ModelCfg.tiny()
    (tmp_path / "cosyvoice3.yaml").write_text(FACADE_YAML)
    for name, m in (("llm", cfg.llm), ("flow", cfg.flow), ("hift", cfg.hift)):
        sd = {k: torch.from_numpy(v) for k, v in synth.state_dict(m.manifest()).items()}
        torch.save({"generator." + k: v for k, v in sd.items()} if name == "hift" else sd, tmp_path / f"{name}.pt")
    model = AutoModel(model_dir=str(tmp_path), frontend=StandInFrontEnd(cfg), max_batch=2, max_tokens=260, max_prompt_tokens=32, sampler="greedy")
    items = [("instruct2", dict(tts_text="你好世界", instruct_text="用四川话说<|endofprompt|>", prompt_wav="prompt.wav")), None,
             ("zero_shot", dict(tts_text="今天天气", prompt_text="提示<|endofprompt|>", prompt_wav="other.wav")),
             ("cross_lingual", dict(tts_text="再见", prompt_wav="third.wav"))]
    alone = [list(getattr(model, "inference_" + it[0])(**it[1]))[0]["tts_speech"] for it in items if it is not None]
    got = list(model.inference_serve(items, group_max=1))
    assert sorted((o["item"], o["segment"]) for o in got) == [(0, 0), (1, 0), (2, 0)]
    for o in got:
        assert o["index"] == o["item"] and torch.equal(o["tts_speech"], alone[o["item"]]), o["item"]
    with pytest.raises(ValueError, match="unknown mode"):
        list(model.inference_serve([("sing", dict(tts_text="x"))]))
