"""CosyVoice3Model.tts_stream_batch: K stream=True utterances through one lane (one LM slot session, one flow stream-slot session).
Each utterance's chunks must be the ones `tts(stream=True)` yields for it alone with the same sampler inputs (greedy): equal
lengths chunk by chunk, equal samples bit for bit."""
import pytest
import torch

from fangyan_tts_amd import synth
from fangyan_tts_amd.spec import ModelCfg
from gpu_util import llm_case, synth_mel

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.mark.parametrize("tag,cases", [("tiny", [(40, 6, 0, 12), (30, 5, 0, 25), (24, 4, 0, 7)]),
                                       ("full", [(8, 8, 0, 25), (6, 5, 0, 12), (7, 4, 0, 30)])])
def test_stream_batch_equals_single_streams(tag, cases):
    from fangyan_tts_amd.cli.model import CosyVoice3Model
    cfg = ModelCfg.tiny() if tag == "tiny" else ModelCfg()
    sd = [synth.state_dict_torch(m.manifest(), DEV, skip=("lm_head",)) for m in (cfg.llm, cfg.flow, cfg.hift)]
    n_text_max = max(c[0] for c in cases)
    ri = torch.from_numpy(synth.hift_rand_ini())
    sn = torch.from_numpy(synth.hift_sine_noise(2 * 20 * n_text_max * 480))
    m = CosyVoice3Model(sd[0], sd[1], sd[2], cfg, device=DEV, max_batch=len(cases), max_text=64, max_prompt_tokens=32, max_tokens=20 * n_text_max,
                        rand_noise=torch.from_numpy(synth.flow_rand_noise(2 * (32 + 20 * n_text_max))), rand_ini=ri, sine_noise=sn)
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
        assert o["tts_speech"].device.type == "cpu" and o["tts_speech"].shape[0] == 1
        got[i].append(o["tts_speech"])
    for i in range(len(inputs)):
        assert [c.shape[1] for c in got[i]] == [c.shape[1] for c in alone[i]], i
        assert len(alone[i]) >= 2, i                                        # at least one streaming chunk before the final pass
        assert torch.equal(torch.cat(got[i], dim=1), torch.cat(alone[i], dim=1)), i
    # the lane is free again and the single-stream path still works on it
    again = [o["tts_speech"] for o in m.tts(**inputs[0], stream=True)]
    assert torch.equal(torch.cat(again, dim=1), torch.cat(alone[0], dim=1))
