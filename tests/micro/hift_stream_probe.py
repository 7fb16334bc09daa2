# The vocoder's share of a stream=True generation, per chunk: full-size HiFT (synthetic weights) through the facade's chunk schedule
# (first hop padded to the 50-frame grid, 50-frame hops, finalize on the whole) for 10 s, 32 s and 64 s of mel, with the incremental
# vocoder (FY_INCREMENTAL: the new frames plus the margin) and the whole-mel form, alternating stream by stream after a warm-up.
# Every call is timed with HIP events on the call's stream (the output allocation included, as in the facade).  Also the
# voice-conversion stream=True path end to end (flow + vocoder chunks, no LM) at 10 s and 32 s, both forms.
#   python tests/micro/hift_stream_probe.py [--rounds 5] [--out FILE.json]   (default: profiles/hift_stream_probe.json)
import argparse, json, os, statistics, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from fangyan_tts_amd import synth
from fangyan_tts_amd.hift import HiftEngine
from fangyan_tts_amd.spec import HiftCfg, ModelCfg

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))),
                                          "profiles", "hift_stream_probe.json"))
ap.add_argument("--no-e2e", action="store_true")
args = ap.parse_args()
dev = torch.device("cuda:0")
UP = 480


def schedule(total, pad=30, hop=50):
    fs, f = [], pad + hop
    while f < total:
        fs.append(f)
        f += hop
    return fs + [total]


cfg = HiftCfg()
sd = synth.state_dict_torch(cfg.manifest(), dev)
eng = HiftEngine(sd, cfg, max_batch=1, max_frames=3200, device=dev)
g = torch.Generator(device="cpu").manual_seed(0)
mel = torch.rand(1, 80, 3200, generator=g).to(dev)
ri = torch.from_numpy(synth.hift_rand_ini()).to(dev)
sn = torch.from_numpy(synth.hift_sine_noise(3200 * UP)).to(dev)
st = torch.cuda.current_stream(dev)


def run(sched, incremental):
    evs, wins = [], []
    eng.stream_reset()
    for i, F in enumerate(sched):
        m = mel[:, :, :F].contiguous()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        eng.inference(m, ri, sn, finalize=i == len(sched) - 1, incremental=incremental)
        b.record(st)
        evs.append((a, b))
        wins.append(eng.stream_window() if incremental else F)
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in evs], wins


rec = {"config": "HiftCfg() full size, synthetic weights, B = 1; ms per vocoder call by HIP events, median over rounds",
       "rounds": args.rounds, "lengths": {}}
for F_total, name in ((500, "10s"), (1600, "32s"), (3200, "64s")):
    sched = schedule(F_total)
    for inc in (True, False):                                   # warm-up
        run(sched, inc)
    t = {True: [], False: []}
    wins = None
    for _ in range(args.rounds):
        for inc in (True, False):                               # alternating
            ms, w = run(sched, inc)
            t[inc].append(ms)
            if inc:
                wins = w
    med = {k: [round(statistics.median(c), 4) for c in zip(*v)] for k, v in t.items()}
    r = {"frames": sched, "window_incremental": wins, "ms_incremental": med[True], "ms_whole": med[False],
         "total_ms_incremental": round(sum(med[True]), 3), "total_ms_whole": round(sum(med[False]), 3)}
    rec["lengths"][name] = r
    n = len(sched)
    pick = sorted({0, 1, n // 2, n - 2, n - 1})
    print(f"{name}: {n} calls; incremental total {r['total_ms_incremental']:.2f} ms, whole-mel total {r['total_ms_whole']:.2f} ms", flush=True)
    for i in pick:
        print(f"   call {i:3d} F {sched[i]:5d}: window {wins[i]:5d}  incremental {med[True][i]:7.3f} ms   whole {med[False][i]:7.3f} ms", flush=True)

if not args.no_e2e:
    # tts(stream=True) through the voice-conversion branch (given tokens, no LM): flow + vocoder per chunk, both vocoder forms
    from fangyan_tts_amd.cli.model import CosyVoice3Model
    mc = ModelCfg()
    sds = [synth.state_dict_torch(m.manifest(), dev, skip=("lm_head",)) for m in (mc.llm, mc.flow, mc.hift)]
    model = CosyVoice3Model(sds[0], sds[1], sds[2], mc, device=dev, max_batch=1, max_text=64, max_prompt_tokens=64, max_tokens=800,
                            rand_ini=torch.from_numpy(synth.hift_rand_ini()), sine_noise=torch.from_numpy(synth.hift_sine_noise(1600 * UP)))
    prompt = {"flow_prompt_speech_token": torch.from_numpy(synth.randint("probe.ptok", (1, 50), 0, 6561)),
              "prompt_speech_feat": torch.from_numpy(synth.normal("probe.pfeat", (1, 100, 80), -5.0, 2.0)),
              "flow_embedding": torch.from_numpy(synth.normal("in.flow.spk", (1, 192)))}
    orig = model.hift.inference

    def whole(*a, incremental=False, **k):
        return orig(*a, **k)
    rec["e2e_vc_stream"] = {}
    for n_tok, name in ((250, "10s"), (800, "32s")):
        src = torch.from_numpy(synth.randint(f"probe.vc.{n_tok}", (1, n_tok), 0, 6561))
        res = {True: [], False: []}
        outs = {}
        for rnd in range(1 + args.rounds):
            for inc in (True, False):
                if inc:
                    model.hift.__dict__.pop("inference", None)
                else:
                    model.hift.inference = whole
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                chunks = [o["tts_speech"] for o in model.tts(source_speech_token=src, stream=True, **prompt)]
                dt = time.perf_counter() - t0
                if rnd:
                    res[inc].append(1e3 * dt)
                outs[inc] = chunks
        model.hift.__dict__.pop("inference", None)
        same = len(outs[True]) == len(outs[False]) and all(torch.equal(a, b) for a, b in zip(outs[True], outs[False]))
        rec["e2e_vc_stream"][name] = {"tokens": n_tok, "chunks": len(outs[True]), "ms_incremental": round(statistics.median(res[True]), 2),
                                      "ms_whole": round(statistics.median(res[False]), 2), "chunks_identical": same}
        print(f"vc stream {name} ({n_tok} tokens, {len(outs[True])} chunks): incremental vocoder {statistics.median(res[True]):.1f} ms, "
              f"whole-mel vocoder {statistics.median(res[False]):.1f} ms, chunks identical: {same}", flush=True)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
json.dump(rec, open(args.out, "w"), indent=1)
print("wrote", args.out)
