# The streaming serving loop against the only way the code before it had to stream several requests on one lane, full size (synthetic
# weights), 4 slots: 16 stream=True requests, text lengths spread over 0.5 .. 1.0 of the benchmark's (5 .. 20 ids; the LM's own
# stopping rule decides the token counts), the benchmark's 5 s prompt.
#   serve_stream: tts_serve_stream (4 slots)
#   stream_batch: tts_stream_batch over arrival-order groups of 4 - a group starts when its last member has arrived and the group
#                 before it has ended
# Two arrival patterns: (a) "present": all 16 at the start; (b) "arriving": one request every other poll of the serving loop.  For
# stream_batch under (b) the arrival times are the offsets from the start at which serve_stream's warm run read each request (the
# loop's polls are its own clock; the baseline has none), and a group waits for its last member's offset.
# Per mode and pattern: total wall time by the host clock, per-request time to the first chunk measured from its arrival, LM token steps
# (the slot sessions' own counters, summed over stream_batch's groups) and chunk passes (FlowEngine.inference_streams calls, counted by
# a wrapper).  One warm run of each, then --runs runs each, alternating; medians with the spread.
#   python tests/micro/serve_stream_probe.py [--runs 3] [--out FILE.json]   (default: profiles/serve_stream_probe.json)
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "serve_stream_probe.json"))
args = ap.parse_args()
dev = torch.device("cuda:0")
cfg = ModelCfg()
MB, N, P_TOK, TEXT_MAX, EVERY = 4, 16, 125, 20, 2
hi = min(cfg.llm.vocab, 151643)
n_text = [int(round(f * (10 + int(synth.randint(f"probe.sstream.len.{i}", (1,), 0, 11)[0])))) for i, f in enumerate(np.linspace(0.5, 1.0, N))]
order = synth.randint("probe.sstream.order", (N,), 0, 1 << 30).argsort().tolist()        # the spread, in a mixed arrival order
n_text = [n_text[i] for i in order]
inputs = []
for i in range(N):
    tag = f"probe.sstream.u{i % MB}"                          # four prompts, presented again and again
    inputs.append({"text": torch.from_numpy(synth.randint(f"probe.sstream.text.{i}", (1, n_text[i]), 0, hi)),
                   "prompt_text": torch.from_numpy(synth.randint(tag + ".instruct", (1, 8), 0, hi)),
                   "llm_prompt_speech_token": torch.zeros(1, 0, dtype=torch.int32),
                   "flow_prompt_speech_token": torch.from_numpy(synth.randint(tag + ".ptok", (1, P_TOK), 0, cfg.flow.vocab)),
                   "prompt_speech_feat": torch.from_numpy(np.clip(synth.normal(tag + ".pfeat", (1, 2 * P_TOK, 80), -5.0, 2.0), -11.5, 2.0)),
                   "flow_embedding": torch.from_numpy(synth.normal(tag + ".spk", (1, 192)))})
for i in range(MB, N):                                        # the same tensor objects: the prompt cache is keyed by identity
    for k in ("prompt_text", "flow_prompt_speech_token", "prompt_speech_feat", "flow_embedding"):
        inputs[i][k] = inputs[i % MB][k]
max_tokens = 20 * TEXT_MAX
sd = [synth.state_dict_torch(m.manifest(), dev, skip=("lm_head",)) for m in (cfg.llm, cfg.flow, cfg.hift)]
m = CosyVoice3Model(sd[0], sd[1], sd[2], cfg, device=dev, max_batch=MB, max_text=64, max_prompt_tokens=P_TOK, max_tokens=max_tokens,
                    rand_noise=torch.from_numpy(synth.flow_rand_noise(2 * (P_TOK + max_tokens))), rand_ini=torch.from_numpy(synth.hift_rand_ini()),
                    sine_noise=torch.from_numpy(synth.hift_sine_noise(2 * max_tokens * 480)))
del sd
chunk_calls = [0]
_streams = m.flow.inference_streams


def counted(*a, **k):
    chunk_calls[0] += 1
    return _streams(*a, **k)


m.flow.inference_streams = counted


def run_serve(arriving):
    """-> (wall s, per request: first-chunk time - arrival time, arrival offsets, token steps, chunk passes, samples per request)"""
    arrived, first, samples = {}, {}, [0] * N
    chunk_calls[0] = 0
    t0 = time.perf_counter()

    def requests():
        for i, d in enumerate(inputs):
            arrived[i] = time.perf_counter() - t0
            yield d
            if arriving:
                for _ in range(EVERY):
                    yield None

    for o in m.tts_serve_stream(requests(), n_slots=MB):
        first.setdefault(o["index"], time.perf_counter() - t0)
        samples[o["index"]] += o["tts_speech"].shape[1]
    wall = time.perf_counter() - t0
    return wall, [first[i] - arrived[i] for i in range(N)], [arrived[i] for i in range(N)], m.last_serve_stream["token_steps"], chunk_calls[0], samples


def run_batch(offsets):
    """offsets: per request its arrival, seconds from the start (None: all present)."""
    first, samples, steps = {}, [0] * N, 0
    chunk_calls[0] = 0
    t0 = time.perf_counter()
    for g in range(0, N, MB):
        if offsets is not None:
            while time.perf_counter() - t0 < offsets[g + MB - 1]:             # the group's last member has not arrived yet
                time.sleep(1e-4)
        for i, o in m.tts_stream_batch(inputs[g: g + MB]):
            first.setdefault(g + i, time.perf_counter() - t0)
            samples[g + i] += o["tts_speech"].shape[1]
        steps += m.lanes[0].llm.slot_steps
    wall = time.perf_counter() - t0
    return wall, [first[i] - (offsets[i] if offsets is not None else 0.0) for i in range(N)], offsets, steps, chunk_calls[0], samples


warm_arriving = run_serve(True)
offsets = warm_arriving[2]
modes = {"present.serve_stream": lambda: run_serve(False), "present.stream_batch": lambda: run_batch(None),
         "arriving.serve_stream": lambda: run_serve(True), "arriving.stream_batch": lambda: run_batch(offsets)}
warm = {name: fn() for name, fn in modes.items()}
assert all(warm[name][5] == warm["present.stream_batch"][5] for name in modes), "the modes delivered different amounts of audio"
runs = {name: [] for name in modes}
for _ in range(args.runs):
    for name, fn in modes.items():
        torch.cuda.synchronize()
        runs[name].append(fn())
        torch.cuda.synchronize()
med = lambda xs: statistics.median(xs)
rec = {"config": f"ModelCfg() full size, synthetic weights, {MB} slots, {N} stream=True requests, text {min(n_text)}..{max(n_text)} ids, {P_TOK} prompt "
                 f"tokens, the LM's own stopping rule (tokens per request {[s // 960 for s in warm['present.stream_batch'][5]]}), 25 tokens per "
                 f"poll; 'arriving': one request every {EVERY} polls of the serving loop, stream_batch given the offsets of serve_stream's warm run; "
                 f"host clock, one warm run of each, then median of {args.runs} alternating runs",
       "arrival_offsets_ms": [round(1e3 * x, 1) for x in offsets], "modes": {}}
for name in modes:
    walls = [1e3 * r[0] for r in runs[name]]
    ttfc = [[1e3 * r[1][i] for r in runs[name]] for i in range(N)]
    ttfc_med = [med(x) for x in ttfc]
    rec["modes"][name] = {"wall_ms": [round(x, 1) for x in walls], "median_ms": round(med(walls), 1), "spread_ms": round(max(walls) - min(walls), 1),
                          "first_chunk_ms_per_request": [round(x, 1) for x in ttfc_med],
                          "first_chunk_ms_median": round(med(ttfc_med), 1), "first_chunk_ms_max": round(max(ttfc_med), 1),
                          "first_chunk_spread_ms_max": round(max(max(x) - min(x) for x in ttfc), 1),
                          "lm_token_steps": warm[name][3], "chunk_passes": warm[name][4]}
    print(name, rec["modes"][name], flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
json.dump(rec, open(args.out, "w"), indent=1)
print("wrote", args.out)
