# The non-stream serving loop against the fixed-batch entry points, full size (synthetic weights), max_batch 8: 64 requests, all present
# at the start, text lengths spread over 0.5 .. 1.0 of the benchmark's (5 .. 20 ids; the LM's own stopping rule decides the token
# counts, 2 x .. 20 x the text length), the benchmark's 5 s prompt.
#   batch:        tts_batch over arrival-order groups of 8
#   pipeline:     tts_pipeline over the same groups
#   serve:        tts_serve (8 slots, groups of up to 8), flow_packed off
#   serve_packed: the same with flow_packed on
# One warm run of each, then --runs runs each, alternating; wall ms by the host clock around calls that end with the audio on the host.
# Also per mode: LM token steps and the rows the flow decoder ran.  MEASURED: serve's token steps (what the slot session launched), batch's
# and serve's flow rows (FlowEngine.last_rows summed over the calls).  DERIVED, and named so in each mode's "derived" list: the token
# steps of batch / pipeline (each group runs to its longest member: from the raw counts of one LM pass per group) and pipeline's flow
# rows (it makes tts_batch's flow calls on the same groups: batch's figure).
#   python tests/micro/serve_probe.py [--runs 3] [--requests 64] [--out FILE.json]   (default: profiles/serve_probe.json)
import argparse, json, os, statistics, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from fangyan_tts_amd import synth
from fangyan_tts_amd.cli.model import CosyVoice3Model
from fangyan_tts_amd.spec import ModelCfg

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--requests", type=int, default=64)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "serve_probe.json"))
args = ap.parse_args()
dev = torch.device("cuda:0")
cfg = ModelCfg()
MB, POLL, N, P_TOK, TEXT_MAX = 8, 8, args.requests, 125, 20
hi = min(cfg.llm.vocab, 151643)
n_text = [int(round(f * (10 + int(synth.randint(f"probe.serve.len.{i}", (1,), 0, 11)[0])))) for i, f in enumerate(np.linspace(0.5, 1.0, N))]
order = synth.randint("probe.serve.order", (N,), 0, 1 << 30).argsort().tolist()          # the spread, in a mixed arrival order
n_text = [n_text[i] for i in order]
inputs = []
for i in range(N):
    tag = f"probe.serve.u{i % MB}"                            # eight prompts, presented again and again (the prompt cache's case)
    inputs.append({"text": torch.from_numpy(synth.randint(f"probe.serve.text.{i}", (1, n_text[i]), 0, hi)),
                   "prompt_text": torch.from_numpy(synth.randint(tag + ".instruct", (1, 8), 0, hi)),
                   "llm_prompt_speech_token": torch.zeros(1, 0, dtype=torch.int32),
                   "flow_prompt_speech_token": torch.from_numpy(synth.randint(tag + ".ptok", (1, P_TOK), 0, cfg.flow.vocab)),
                   "prompt_speech_feat": torch.from_numpy(np.clip(synth.normal(tag + ".pfeat", (1, 2 * P_TOK, 80), -5.0, 2.0), -11.5, 2.0)),
                   "flow_embedding": torch.from_numpy(synth.normal(tag + ".spk", (1, 192)))})
for i in range(MB, N):                                        # the same tensor objects: the cache is keyed by identity
    for k in ("prompt_text", "flow_prompt_speech_token", "prompt_speech_feat", "flow_embedding"):
        inputs[i][k] = inputs[i % MB][k]
groups = [inputs[g: g + MB] for g in range(0, N, MB)]
max_tokens = 20 * TEXT_MAX
sd = [synth.state_dict_torch(m.manifest(), dev, skip=("lm_head",)) for m in (cfg.llm, cfg.flow, cfg.hift)]
m = CosyVoice3Model(sd[0], sd[1], sd[2], cfg, device=dev, max_batch=MB, max_text=64, max_prompt_tokens=P_TOK, max_tokens=max_tokens,
                    rand_noise=torch.from_numpy(synth.flow_rand_noise(2 * (P_TOK + max_tokens))), rand_ini=torch.from_numpy(synth.hift_rand_ini()),
                    sine_noise=torch.from_numpy(synth.hift_sine_noise(2 * max_tokens * 480)))
del sd
z = torch.zeros(1, 0, dtype=torch.int32)
raw = []
for g in groups:
    _, _, r = m.llm.generate([d["text"].reshape(-1).tolist() for d in g], [d["prompt_text"].reshape(-1).tolist() for d in g], [[] for _ in g])
    raw += r.cpu().tolist()
steps_grouped = sum(max(raw[g: g + MB]) - 1 for g in range(0, N, MB))


def run_batch():
    rows, toks = 0, []
    for g in groups:
        _, _, t = m.tts_batch(g)
        rows += m.flow.last_rows
        toks += [x.cpu().tolist() for x in t]
    return toks, steps_grouped, rows


def run_pipeline():
    toks = []
    for _, _, t in m.tts_pipeline(groups):
        toks += [x.cpu().tolist() for x in t]
    return toks, steps_grouped, None


def run_serve(packed):
    m.flow_packed = packed
    try:
        got = {o["index"]: o["tokens"].cpu().tolist() for o in m.tts_serve(inputs, steps_per_poll=POLL)}
    finally:
        m.flow_packed = False
    return [got[i] for i in range(N)], m.last_serve["token_steps"], m.last_serve["flow_rows"]


modes = {"batch": run_batch, "pipeline": run_pipeline, "serve": lambda: run_serve(False), "serve_packed": lambda: run_serve(True)}
rec = {"config": f"ModelCfg() full size, synthetic weights, max_batch {MB}, {N} requests present at the start, text {min(n_text)}..{max(n_text)} ids, "
                 f"{P_TOK} prompt tokens, the LM's own stopping rule (raw counts {min(raw)}..{max(raw)}, sum {sum(raw)}), {POLL} token steps per poll, "
                 f"group_wait 2; wall ms by the host clock, median of {args.runs} alternating runs after one warm run of each",
       "note": "wall_ms, median_ms, spread_ms, requests_per_s and ids_equal_batch are measured; of lm_token_steps and flow_rows, the fields a "
               "mode lists under 'derived' are computed (batch / pipeline token steps: sum over groups of the longest raw count - 1; pipeline "
               "flow rows: batch's, the same flow calls) and the others are counted by the run",
       "raw_counts": raw, "modes": {}}
warm = {name: fn() for name, fn in modes.items()}
ids_same = {name: warm[name][0] == warm["batch"][0] for name in modes}
t = {name: [] for name in modes}
for _ in range(args.runs):
    for name, fn in modes.items():
        torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
        t[name].append(1e3 * (time.perf_counter() - t0))
rows_batch = warm["batch"][2]
for name in modes:
    med = statistics.median(t[name])
    rec["modes"][name] = {"wall_ms": [round(x, 1) for x in t[name]], "median_ms": round(med, 1), "spread_ms": round(max(t[name]) - min(t[name]), 1),
                          "requests_per_s": round(N / (med * 1e-3), 2), "lm_token_steps": warm[name][1],
                          "flow_rows": warm[name][2] if warm[name][2] is not None else rows_batch, "ids_equal_batch": ids_same[name],
                          "derived": {"batch": ["lm_token_steps"], "pipeline": ["lm_token_steps", "flow_rows"]}.get(name, [])}
    print(name, rec["modes"][name], flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
json.dump(rec, open(args.out, "w"), indent=1)
print("wrote", args.out)
