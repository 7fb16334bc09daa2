# Flow stream slots: one batched chunk pass for K streams (FlowEngine.inference_streams) against what K single-stream incremental
# calls cost - (a) one after another, (b) from K threads on K streams - each stream on a handle of its own.  Full size, 5 s prompt
# (125 tokens), 10 s of audio per stream (250 tokens = 10 polls).  HIP-event time per poll; median of three runs after a warm one,
# legs alternated.  Writes profiles/flow_stream_slots_probe.json.   python tests/micro/flow_stream_slots_probe.py [K ...]
import json, os, statistics, sys, threading, torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from fangyan_tts_amd import synth
from fangyan_tts_amd.flow import FlowEngine
from fangyan_tts_amd.spec import FlowCfg
cfg = FlowCfg(); dev = torch.device("cuda:0")
HOP, LOOK, P, POLLS = 25, 3, 125, 10
CAP = 2 * (P + POLLS * HOP)
Ks = [int(a) for a in sys.argv[1:]] or [1, 2, 4, 8]
sd = synth.state_dict_torch(cfg.manifest(), dev)
noise = torch.from_numpy(synth.flow_rand_noise(CAP)).to(dev)
engs = [FlowEngine(sd, cfg, max_batch=1, max_frames=CAP, device=dev) for _ in range(max(Ks))]
free0 = torch.cuda.mem_get_info()[0]
tok = [torch.from_numpy(synth.randint(f"probe.slots.tok.{i}", (1, POLLS * HOP + LOOK), 0, cfg.vocab)).to(dev) for i in range(max(Ks))]
ptok = [torch.from_numpy(synth.randint(f"probe.slots.ptok.{i}", (1, P), 0, cfg.vocab)).to(dev) for i in range(max(Ks))]
pfeat = [torch.from_numpy(synth.uniform(f"probe.slots.pfeat.{i}", (1, 2 * P, 80), -6.0, 2.0)).to(dev) for i in range(max(Ks))]
emb = [torch.from_numpy(synth.normal(f"probe.slots.spk.{i}", (1, cfg.spk_in))).to(dev) for i in range(max(Ks))]
streams = [torch.cuda.Stream(device=dev) for _ in range(max(Ks))]

def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); a.record(); fn(); b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b)

def one(i, k):
    n = k * HOP + LOOK
    return engs[i].inference(tok[i][:, :n], [n], ptok[i], [P], pfeat[i], [2 * P], emb[i], noise, streaming=True, finalize=False, incremental=True)

def leg_batched(K):
    for s in range(K): engs[0].stream_slot_reset(s)
    out = []
    for k in range(1, POLLS + 1):
        n = k * HOP + LOOK
        out.append(timed(lambda: engs[0].inference_streams(list(range(K)), torch.cat([t[:, :n] for t in tok[:K]]), [n] * K, torch.cat(ptok[:K]), [P] * K,
                                                           torch.cat(pfeat[:K]), [2 * P] * K, torch.cat(emb[:K]), noise)))
    return out

def leg_serial(K):
    for i in range(K): engs[i].stream_reset()
    return [timed(lambda: [one(i, k) for i in range(K)]) for k in range(1, POLLS + 1)]

def leg_threads(K):
    for i in range(K): engs[i].stream_reset()
    out = []
    for k in range(1, POLLS + 1):
        def job(i):
            with torch.cuda.device(dev), torch.cuda.stream(streams[i]):
                one(i, k)
        def fn():
            cur = torch.cuda.current_stream(dev)
            for i in range(K): streams[i].wait_stream(cur)
            th = [threading.Thread(target=job, args=(i,)) for i in range(K)]
            [t.start() for t in th]; [t.join() for t in th]
            for i in range(K): cur.wait_stream(streams[i])
        out.append(timed(fn))
    return out

res = {"config": {"prompt_tokens": P, "polls": POLLS, "hop": HOP, "frames_per_slot": CAP, "audio_s_per_stream": POLLS * HOP * 2 * 480 / 24000.0}, "K": {}}
for K in Ks:
    engs[0].open_streams(K, CAP)
    legs = {"batched": leg_batched, "serial_single": leg_serial, "threads_single": leg_threads}
    runs = {name: [] for name in legs}
    for r in range(4):                                       # run 0 warms
        for name, fn in legs.items():
            t = fn(K)
            if r: runs[name].append(t)
    row = {"session_bytes": engs[0].streams_bytes}
    for name, rs in runs.items():
        per_poll = [statistics.median(x) for x in zip(*rs)]
        tot = sorted(sum(x) for x in rs)
        row[name] = {"ms_per_poll_first_last": [round(per_poll[0], 2), round(per_poll[-1], 2)], "ms_per_poll_median": round(statistics.median(per_poll), 2),
                     "ms_all_polls_median": round(tot[1], 1), "ms_all_polls_min_max": [round(tot[0], 1), round(tot[-1], 1)],
                     "ms_per_stream_second_of_audio": round(tot[1] / (K * res["config"]["audio_s_per_stream"]), 2)}
    res["K"][str(K)] = row
    engs[0].close_streams()
    print(K, json.dumps(row), flush=True)
res["handle_bytes_saved_per_extra_stream"] = "one FlowEngine's allocations (weights + folded tables); see free_bytes_after_handles"
res["free_bytes_after_handles"] = free0
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
json.dump(res, open(os.path.join(ROOT, "profiles", "flow_stream_slots_probe.json"), "w"), indent=1)
