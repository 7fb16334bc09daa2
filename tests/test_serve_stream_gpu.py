"""The streaming serving loop (CosyVoice3Model.tts_serve_stream): stream=True requests join slots over time on one lane.

Yardsticks: per request the chunks `tts(**request, stream=True)` yields for it alone (greedy sampling) - equal lengths chunk by chunk,
equal samples with torch.equal - and `plan_serve_stream` for the schedule.  There is no tolerance in this file."""
import threading
import time

import pytest
import torch

from fangyan_tts_amd import synth
from fangyan_tts_amd._lib import FY_PRECISE, HOST_WAIT_SLEEP_S
from fangyan_tts_amd.flow import plan_serve_stream
from fangyan_tts_amd.spec import ModelCfg
from gpu_util import llm_case, synth_mel

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SLOTS = 2
# (text ids, prompt-text ids, LM prompt speech tokens, flow prompt tokens) per request: through 2 slots these force slot reuse, a join
# beside a running stream, two streams ending in one poll and at least one streaming chunk before each final pass.
# Two texts are longer than first planned: with 12 ids the tiny model's fourth request stopped after 29 tokens and with 8 ids the full
# model's first after fewer than 28 - one final pass and no streaming chunk.  The LM emits at least 2 tokens per text id, so 21 ids
# reach the 25 + 13 + 3 tokens of a first chunk behind a 12-token prompt, and 14 ids the 25 + 3 behind a 25-token one.
CASES = {"tiny": [(40, 6, 0, 12), (30, 5, 0, 25), (24, 4, 10, 7), (21, 3, 0, 12), (36, 5, 6, 25)],
         "full": [(14, 8, 0, 25), (6, 5, 0, 12), (7, 4, 5, 30)]}
_worlds = {}


class World:
    """One model per configuration for the whole module, its requests and what each request streams alone."""

    def __init__(self, tag):
        from fangyan_tts_amd.cli.model import CosyVoice3Model
        cases = CASES[tag]
        cfg = ModelCfg.tiny() if tag == "tiny" else ModelCfg()
        sd = [synth.state_dict_torch(m.manifest(), DEV, skip=("lm_head",)) for m in (cfg.llm, cfg.flow, cfg.hift)]
        n_text_max = max(c[0] for c in cases)
        self.m = CosyVoice3Model(sd[0], sd[1], sd[2], cfg, device=DEV, max_batch=SLOTS, max_text=64, max_prompt_tokens=32,
                                 max_tokens=20 * n_text_max, rand_noise=torch.from_numpy(synth.flow_rand_noise(2 * (32 + 20 * n_text_max))),
                                 rand_ini=torch.from_numpy(synth.hift_rand_ini()),
                                 sine_noise=torch.from_numpy(synth.hift_sine_noise(2 * 20 * n_text_max * 480)))
        self.inputs = []
        for n_text, n_ptext, p_llm, p_flow in cases:
            t, pt, pk = llm_case(cfg.llm, n_text, n_ptext, p_llm, f"sstream.{n_text}_{n_ptext}_{p_llm}_{p_flow}")
            self.inputs.append({
                "text": torch.tensor([t], dtype=torch.int32), "prompt_text": torch.tensor([pt], dtype=torch.int32),
                "llm_prompt_speech_token": torch.tensor([pk], dtype=torch.int32).reshape(1, -1),
                "flow_prompt_speech_token": torch.from_numpy(synth.randint(f"in.flow.ptoken.sstream.{p_flow}", (1, p_flow), 0, 6561)),
                "prompt_speech_feat": torch.from_numpy(synth_mel(f"in.flow.pfeat.sstream.{p_flow}", 2 * p_flow)),
                "flow_embedding": torch.from_numpy(synth.normal(f"in.flow.spk.sstream.{p_flow}", (1, 192))),
            })
        self.p_flow = [c[3] for c in cases]
        self.m.decode_mode_at_rest = self.m.lanes[0].llm.decode_mode
        self._alone = {}

    def alone(self, flags=0):
        """Per request the chunks of tts(stream=True) with flow_flags = flags."""
        if flags not in self._alone:
            self.m.flow_flags = flags
            try:
                self._alone[flags] = [[o["tts_speech"] for o in self.m.tts(**inp, stream=True)] for inp in self.inputs]
            finally:
                self.m.flow_flags = 0
        return self._alone[flags]

    def check(self, got, alone, which=None):
        """got: the loop's items.  Every request: its chunks in order, numbered, the last one final, equal to the solo stream's."""
        which = range(len(self.inputs)) if which is None else which
        assert not any("error" in o for o in got), [o for o in got if "error" in o]
        for i in which:
            print(f"request {i}: chunk samples {[o['tts_speech'].shape[1] for o in got if o['index'] == i]} alone {[c.shape[1] for c in alone[i]]}")
        for i in which:
            mine = [o for o in got if o["index"] == i]
            assert [o["chunk"] for o in mine] == list(range(len(mine))) and [o["final"] for o in mine] == [False] * (len(mine) - 1) + [True], i
            assert all(o["tts_speech"].device.type == "cpu" and o["tts_speech"].shape[0] == 1 for o in mine)
            assert len(alone[i]) >= 2, i                       # at least one streaming chunk before the final pass
            assert [o["tts_speech"].shape[1] for o in mine] == [c.shape[1] for c in alone[i]], i
            assert torch.equal(torch.cat([o["tts_speech"] for o in mine], dim=1), torch.cat(alone[i], dim=1)), i
        assert sorted({o["index"] for o in got}) == sorted(which)


def world(tag) -> World:
    if tag not in _worlds:
        _worlds[tag] = World(tag)
    return _worlds[tag]


def clean(m):
    ln = m.lanes[0]
    assert m._free.qsize() == len(m.lanes)                     # the lane is back
    assert ln.flow.streams_bytes == 0 and ln.hift.streams_bytes() == 0
    assert ln.llm.decode_mode == m.decode_mode_at_rest


# ---------------------------------------------------------------------------------------------------------------- 1. bits
@pytest.mark.parametrize("tag", ["tiny", "full"])
def test_chunks_equal_each_request_streamed_alone(tag):
    w = world(tag)
    alone = w.alone()
    got = list(w.m.tts_serve_stream(w.inputs, record_polls=True))
    w.check(got, alone)
    st = w.m.last_serve_stream
    polls = st["polls"]
    joins = [j for p in polls for j in p["joins"]]
    assert [r for r, _ in joins] == list(range(len(w.inputs))) and len(joins) > SLOTS          # slots were reused
    held, beside = set(), False
    for p in polls:
        beside |= bool(p["joins"]) and bool(held)              # a join beside a running stream
        held |= {s for _, s in p["joins"]}
        held -= set(p["released"])
    assert beside and not held
    assert st["n_polls"] == len(polls) and st["n_joins"] == len(joins)
    assert st["chunk_passes"] == sum(any(not c[3] for c in p["chunks"]) for p in polls)
    assert st["final_passes"] == sum(any(c[3] for c in p["chunks"]) for p in polls)
    assert st["pushes"] == st["chunk_passes"] + st["final_passes"]
    assert 0 < st["token_steps"] <= 25 * len(polls)
    clean(w.m)


# ---------------------------------------------------------------------------------------------------------------- 2. arrival over time
def test_arrivals_over_time_follow_the_plan():
    w = world("tiny")
    alone = w.alone()

    def arriving():
        yield w.inputs[0]
        yield None
        yield w.inputs[1]
        yield None
        yield None
        yield from w.inputs[2:]

    got = list(w.m.tts_serve_stream(arriving(), record_polls=True))
    w.check(got, alone)
    # the lengths that came out: 2 mel frames and 960 samples per token
    n_tok = [sum(c.shape[1] for c in a) // 960 for a in alone]
    # a None ends a poll's arrivals: request 0 in poll 0, request 1 in poll 1, nothing in poll 2, the rest in poll 3
    plan = plan_serve_stream(n_tok, w.p_flow, [0, 1, 3, 3, 3], SLOTS)
    assert w.m.last_serve_stream["polls"] == plan
    assert any(sum(c[3] for c in p["chunks"]) >= 2 for p in plan)                               # two streams end in one poll
    assert any(p["joins"] and any(not c[3] for c in p["chunks"]) for p in plan)                 # a join in a poll that also cuts a chunk
    clean(w.m)


# ---------------------------------------------------------------------------------------------------------------- 3. modes
@pytest.mark.parametrize("mode", ["precise", "packed"])
def test_precise_and_packed_equal_the_solo_stream_in_the_same_mode(mode):
    w = world("tiny")
    m = w.m
    flags = FY_PRECISE if mode == "precise" else 0
    alone = w.alone(flags)
    m.flow_flags, m.flow_packed = flags, mode == "packed"
    try:
        got = list(m.tts_serve_stream(w.inputs))
    finally:
        m.flow_flags, m.flow_packed = 0, False
    w.check(got, alone)
    if mode == "precise":                                      # the mode is not a no-op
        assert not torch.equal(torch.cat(alone[0], dim=1), torch.cat(w.alone()[0], dim=1))
    clean(m)


# ---------------------------------------------------------------------------------------------------------------- 4. errors
def test_request_over_capacity_yields_an_error_item():
    w = world("tiny")
    big = dict(w.inputs[3], text=torch.zeros(1, 65, dtype=torch.int32))                        # max_text is 64
    got = list(w.m.tts_serve_stream([w.inputs[3], big, w.inputs[2]]))
    errs = [o for o in got if "error" in o]
    assert [o["index"] for o in errs] == [1] and isinstance(errs[0]["error"], ValueError)
    alone = w.alone()
    for index, i in ((0, 3), (2, 2)):
        mine = [o["tts_speech"] for o in got if o["index"] == index]
        assert torch.equal(torch.cat(mine, dim=1), torch.cat(alone[i], dim=1)), i
    clean(w.m)


# ---------------------------------------------------------------------------------------------------------------- 5. clean exit
def test_abandoned_generator_leaves_the_model_clean():
    w = world("tiny")
    m = w.m
    alone = w.alone()
    speech = next(m.tts(**w.inputs[1]))["tts_speech"]
    served = {o["index"]: o["tts_speech"] for o in m.tts_serve(w.inputs[:2], group_max=1)}
    n_threads = threading.active_count()
    gen = m.tts_serve_stream(w.inputs)
    first = next(gen)
    assert first["chunk"] == 0 and torch.equal(first["tts_speech"], alone[first["index"]][0])
    gen.close()
    clean(m)
    assert threading.active_count() == n_threads
    again = [o["tts_speech"] for o in m.tts(**w.inputs[0], stream=True)]
    assert torch.equal(torch.cat(again, dim=1), torch.cat(alone[0], dim=1))
    assert torch.equal(next(m.tts(**w.inputs[1]))["tts_speech"], speech)
    after = {o["index"]: o["tts_speech"] for o in m.tts_serve(w.inputs[:2], group_max=1)}
    assert all(torch.equal(after[i], served[i]) for i in (0, 1))
    m.lanes[0].llm.open_slots(8)
    assert m.lanes[0].llm.live() == []
    clean(m)


# ---------------------------------------------------------------------------------------------------------------- 6. idle input
def test_idle_polls_sleep_and_keep_no_record():
    w = world("tiny")
    alone = w.alone()
    t, IDLE_S = {}, 0.02

    def arriving():
        yield w.inputs[3]
        while not t.get("final"):                             # nothing more until the first request has ended
            yield None
        before, end = w.m.last_serve_stream["n_polls"], time.monotonic() + IDLE_S
        while time.monotonic() < end:                         # nothing running, nothing arriving
            yield None
        t["polls idle"] = w.m.last_serve_stream["n_polls"] - before
        t["state"] = dict(w.m.last_serve_stream)
        yield w.inputs[2]

    got = []
    for o in w.m.tts_serve_stream(arriving()):
        got.append(o)
        t["final"] = o["final"]
    assert [o["index"] for o in got if o["final"]] == [0, 1]
    for index, i in ((0, 3), (1, 2)):
        assert torch.equal(torch.cat([o["tts_speech"] for o in got if o["index"] == index], dim=1), torch.cat(alone[i], dim=1))
    st = w.m.last_serve_stream
    assert "polls" not in st and st["n_joins"] == 2
    assert all(isinstance(v, int) for v in st.values()) and set(st) == set(t["state"])        # counters only, before and after
    # every idle poll sleeps at least the interval: no more than IDLE_S / interval of them (a spinning loop makes thousands)
    assert 1 <= t["polls idle"] <= IDLE_S / HOST_WAIT_SLEEP_S + 2, t
    clean(w.m)


# ---------------------------------------------------------------------------------------------------------------- 7. the facade
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
        ids = lambda text, n: torch.from_numpy(synth.randint("sstream.fe." + text, (1, n), 0, self.cfg.llm.vocab))
        tok = torch.from_numpy(synth.randint("sstream.fe.tok." + prompt_wav, (1, p), 0, 6561))
        emb = torch.from_numpy(synth.normal("sstream.fe.spk." + prompt_wav, (1, 192)))
        return {"text": ids(tts_text, 5 + len(tts_text)), "prompt_text": ids(prompt_text, 5), "llm_prompt_speech_token": tok,
                "flow_prompt_speech_token": tok, "prompt_speech_feat": torch.from_numpy(synth_mel("sstream.fe.feat." + prompt_wav, 2 * p)),
                "llm_embedding": emb, "flow_embedding": emb}

    def frontend_instruct2(self, tts_text, instruct_text, prompt_wav, resample_rate, zero_shot_spk_id):
        d = self.frontend_zero_shot(tts_text, instruct_text, prompt_wav, resample_rate, zero_shot_spk_id)
        del d["llm_prompt_speech_token"]
        return d

    def frontend_cross_lingual(self, tts_text, prompt_wav, resample_rate, zero_shot_spk_id):
        d = self.frontend_zero_shot(tts_text, "", prompt_wav, resample_rate, zero_shot_spk_id)
        del d["prompt_text"], d["llm_prompt_speech_token"]
        return d


def test_facade_inference_serve_stream(tmp_path):
    """CosyVoice3.inference_serve(stream=True): (mode, kwargs) items, a None between them, through two slots -> each item's chunks
    are those of its own inference_*(stream=True) call, with the item's position attached."""
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
    alone = [[o["tts_speech"] for o in getattr(model, "inference_" + it[0])(**it[1], stream=True)] for it in items if it is not None]
    got = list(model.inference_serve(items, stream=True))
    assert sorted({(o["item"], o["segment"]) for o in got}) == [(0, 0), (1, 0), (2, 0)]
    for k in range(3):
        mine = [o for o in got if o["item"] == k]
        assert all(o["index"] == k for o in mine) and [o["chunk"] for o in mine] == list(range(len(mine))) and mine[-1]["final"]
        assert [o["tts_speech"].shape[1] for o in mine] == [c.shape[1] for c in alone[k]], k
        assert torch.equal(torch.cat([o["tts_speech"] for o in mine], dim=1), torch.cat(alone[k], dim=1)), k
    with pytest.raises(ValueError, match="unknown mode"):
        list(model.inference_serve([("sing", dict(tts_text="x"))], stream=True))
