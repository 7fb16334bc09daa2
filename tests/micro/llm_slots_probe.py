# Decode slots against the grouped schedule, full-size LM (synthetic weights), max_batch 32: 128 requests of forced lengths drawn once
# from synth between 25 and 250 tokens (1 to 10 s of audio) behind a prompt of 40 speech tokens, one weight plane and two.
#   grouped:    LlmEngine.generate over arrival-order groups of 32 (the only way without slots)
#   continuous: LlmEngine.generate_continuous (join into the lowest free slots, 8 token steps per poll, release, refill)
# Same handle, same stream, one warm run of each, then three runs each, alternating; wall ms by the host clock around calls that end
# in a stream wait.  Also what a join costs the sequences already running: a poll of 8 steps with a one-sequence join in front
# of it against one without, at 8 and at 24 running rows.
#   python tests/micro/llm_slots_probe.py [--runs 3] [--requests 128] [--out FILE.json]   (default: profiles/llm_slots_probe.json)
import argparse, json, os, statistics, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from fangyan_tts_amd import synth
from fangyan_tts_amd.llm import LlmEngine, grouped_steps, plan_slots
from fangyan_tts_amd.spec import LlmCfg

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--requests", type=int, default=128)
ap.add_argument("--planes", default="1,2")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "llm_slots_probe.json"))
args = ap.parse_args()
dev = torch.device("cuda:0")
cfg = LlmCfg()
MB, POLL, N = 32, 8, args.requests
N_TEXT, N_PTEXT, N_PTOK = 14, 10, 40
lens = synth.randint("probe.slots.len", (N,), 25, 251).tolist()
hi = 151643
texts = [synth.randint(f"probe.slots.text.{i}", (1, N_TEXT), 0, hi)[0].tolist() for i in range(N)]
ptexts = [synth.randint(f"probe.slots.ptext.{i}", (1, N_PTEXT), 0, hi)[0].tolist() for i in range(N)]
ptoks = [synth.randint(f"probe.slots.ptok.{i}", (1, N_PTOK), 0, cfg.speech_tokens)[0].tolist() for i in range(N)]
max_ctx = 2 + N_TEXT + N_PTEXT + N_PTOK + 250 + 2

steps_plan, joins = plan_slots(lens, MB, POLL)
need = [n - 1 for n in lens]
steps_generate = sum(max(need[g: g + MB]) for g in range(0, N, MB))
rec = {"config": f"LlmCfg() full size, synthetic weights, max_batch {MB}, {N} requests, forced lengths 25..250 (sum {sum(lens)}), "
                 f"prompt {N_PTOK} speech tokens + {N_PTEXT + N_TEXT} text ids, {POLL} token steps per poll; wall ms by the host clock, median of "
                 f"{args.runs} alternating runs after one warm run of each",
       "lengths": lens,
       "token_steps": {"continuous_plan": steps_plan, "joins": len(joins), "grouped_polled": grouped_steps(lens, MB, POLL),
                       "grouped_generate": steps_generate},
       # rows that still produce a token, per token step launched
       "mean_useful_rows_per_step": {"continuous": round(sum(need) / steps_plan, 2), "grouped": round(sum(need) / steps_generate, 2)},
       "planes": {}}


def wait():
    torch.cuda.current_stream(dev).synchronize()


def grouped(eng):
    ids = []
    for g in range(0, N, MB):
        s = slice(g, g + MB)
        out, out_n, _ = eng.generate(texts[s], ptexts[s], ptoks[s], min_len=lens[s], max_len=lens[s])
        out, out_n = out.cpu(), out_n.cpu().tolist()
        ids += [out[b, : out_n[b]].tolist() for b in range(len(out_n))]
    return ids


def continuous(eng):
    ids, raw = eng.generate_continuous(texts, ptexts, ptoks, min_len=lens, max_len=lens, steps_per_poll=POLL)
    assert raw == lens
    return ids


def join_cost(eng, live, reps=7):
    """ms of a poll of 8 steps with `live` running rows, alone and with a one-sequence join (into slot `live`) in front of it"""
    eng.open_slots(256)
    idx = list(range(live))
    eng.join(idx, [texts[i] for i in idx], [ptexts[i] for i in idx], [ptoks[i] for i in idx], min_len=[250] * live, max_len=[250] * live)
    eng.step(POLL)
    t = {"poll": [], "join+poll": []}
    for r in range(reps + 1):
        wait(); t0 = time.perf_counter(); eng.step(POLL); a = 1e3 * (time.perf_counter() - t0)
        wait(); t0 = time.perf_counter()
        eng.join([live], [texts[live]], [ptexts[live]], [ptoks[live]], min_len=[250], max_len=[250]); eng.step(POLL)
        b = 1e3 * (time.perf_counter() - t0)
        eng.release(live)
        if r:                                                 # the first round warms the shapes
            t["poll"].append(a); t["join+poll"].append(b)
    return {k: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)} for k, v in t.items()}


for planes in [int(p) for p in args.planes.split(",")]:
    if planes == 2:
        with synth.unrounded_weights():
            sd = synth.state_dict_torch(cfg.manifest(), dev, skip=("lm_head",))
    else:
        sd = synth.state_dict_torch(cfg.manifest(), dev, skip=("lm_head",))
    eng = LlmEngine(sd, cfg, max_batch=MB, max_ctx=max_ctx, weight_planes=planes)
    del sd
    assert eng.weight_planes == planes
    ref = grouped(eng)                                        # warm, and the ids to compare
    got = continuous(eng)
    same = got == ref
    steps_run = eng.slot_steps
    t = {"grouped": [], "continuous": []}
    for _ in range(args.runs):
        for name, fn in (("grouped", grouped), ("continuous", continuous)):
            wait(); t0 = time.perf_counter(); fn(eng); wait()
            t[name].append(1e3 * (time.perf_counter() - t0))
    r = {"ids_identical": same, "token_steps_run_continuous": steps_run, "decode_mode": eng.decode_mode}
    for name, v in t.items():
        med = statistics.median(v)
        r[name] = {"wall_ms": [round(x, 1) for x in v], "median_ms": round(med, 1), "spread_ms": round(max(v) - min(v), 1),
                   "tokens_per_s": round(sum(lens) / (med * 1e-3), 1)}
    r["join_cost"] = {f"{live}_running_rows": join_cost(eng, live) for live in (8, 24)}
    rec["planes"][str(planes)] = r
    print(f"planes {planes}: ids identical {same}; token steps run {steps_run} (plan {steps_plan}, grouped {steps_generate}); "
          f"grouped {r['grouped']['median_ms']} ms, continuous {r['continuous']['median_ms']} ms; join cost {r['join_cost']}", flush=True)
    assert steps_run == steps_plan
    eng.close()
    del eng
    torch.cuda.empty_cache()

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
json.dump(rec, open(args.out, "w"), indent=1)
print("wrote", args.out)
