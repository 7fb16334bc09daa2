# The fp32-class (FY_PRECISE) flow decoder on the streaming side, full size, 5 s prompt (125 tokens), HIP-event time, one warm run
# then the median of three:
#   (1) a B = 1 stream of 10 and of 32 chunks, incremental=True against incremental=False (the full recompute of every chunk: what a
#       precise chunk cost before the split arithmetic had an incremental form);
#   (2) one 4-stream batched call per poll (FlowEngine.inference_streams) against four single-stream incremental calls in series,
#       each stream on a handle of its own, 10 polls.
# Writes profiles/flow_precise_stream_probe.json.   python tests/micro/flow_precise_stream_probe.py
import json, os, statistics, sys, torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from fangyan_tts_amd import synth
from fangyan_tts_amd._lib import FY_PRECISE
from fangyan_tts_amd.flow import FlowEngine
from fangyan_tts_amd.spec import FlowCfg
cfg = FlowCfg(); dev = torch.device("cuda:0")
HOP, LOOK, P, K = 25, 3, 125, 4
CHUNKS = (10, 32)
CAP = 2 * (P + max(CHUNKS) * HOP)
sd = synth.state_dict_torch(cfg.manifest(), dev)
noise = torch.from_numpy(synth.flow_rand_noise(CAP)).to(dev)
engs = [FlowEngine(sd, cfg, max_batch=1, max_frames=CAP if i == 0 else 2 * (P + 10 * HOP), device=dev) for i in range(K)]
tok = [torch.from_numpy(synth.randint(f"probe.pslots.tok.{i}", (1, max(CHUNKS) * HOP + LOOK), 0, cfg.vocab)).to(dev) for i in range(K)]
ptok = [torch.from_numpy(synth.randint(f"probe.pslots.ptok.{i}", (1, P), 0, cfg.vocab)).to(dev) for i in range(K)]
pfeat = [torch.from_numpy(synth.uniform(f"probe.pslots.pfeat.{i}", (1, 2 * P, 80), -6.0, 2.0)).to(dev) for i in range(K)]
emb = [torch.from_numpy(synth.normal(f"probe.pslots.spk.{i}", (1, cfg.spk_in))).to(dev) for i in range(K)]

def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); a.record(); fn(); b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b)

def one(i, k, inc):
    n = k * HOP + LOOK
    return engs[i].inference(tok[i][:, :n].contiguous(), [n], ptok[i], [P], pfeat[i], [2 * P], emb[i], noise, streaming=True, finalize=False,
                             incremental=inc, flags=FY_PRECISE)

def leg_stream(chunks, inc):
    engs[0].stream_reset()
    return [timed(lambda: one(0, k, inc)) for k in range(1, chunks + 1)]

def leg_batched(polls):
    for s in range(K): engs[0].stream_slot_reset(s)
    out = []
    for k in range(1, polls + 1):
        n = k * HOP + LOOK
        out.append(timed(lambda: engs[0].inference_streams(list(range(K)), torch.cat([t[:, :n] for t in tok]), [n] * K, torch.cat(ptok), [P] * K,
                                                           torch.cat(pfeat), [2 * P] * K, torch.cat(emb), noise, flags=FY_PRECISE)))
    return out

def leg_serial(polls):
    for i in range(K): engs[i].stream_reset()
    return [timed(lambda: [one(i, k, True) for i in range(K)]) for k in range(1, polls + 1)]

def measure(legs):
    runs = {name: [] for name in legs}
    for r in range(4):                                       # run 0 warms
        for name, fn in legs.items():
            t = fn()
            if r: runs[name].append(t)
    row = {}
    for name, rs in runs.items():
        per = [statistics.median(x) for x in zip(*rs)]
        tot = sorted(sum(x) for x in rs)
        row[name] = {"ms_per_call_first_last": [round(per[0], 2), round(per[-1], 2)], "ms_all_calls_median": round(tot[1], 1),
                     "ms_all_calls_min_max": [round(tot[0], 1), round(tot[-1], 1)]}
    return row

res = {"config": {"mode": "FY_PRECISE", "prompt_tokens": P, "hop": HOP, "streams_batched": K}, "single_stream": {}, "slots": {}}
for chunks in CHUNKS:
    row = measure({"incremental": lambda: leg_stream(chunks, True), "full_recompute": lambda: leg_stream(chunks, False)})
    res["single_stream"][str(chunks)] = row
    print(chunks, json.dumps(row), flush=True)
engs[0].open_streams(K, 2 * (P + 10 * HOP), precise=True)
row = measure({"batched": lambda: leg_batched(10), "serial_single": lambda: leg_serial(10)})
row["session_bytes"] = engs[0].streams_bytes
engs[0].close_streams()
res["slots"]["10_polls"] = row
print("slots", json.dumps(row), flush=True)
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
json.dump(res, open(os.path.join(ROOT, "profiles", "flow_precise_stream_probe.json"), "w"), indent=1)
