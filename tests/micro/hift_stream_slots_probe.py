# One vocoder pass per poll against one per stream: full-size HiFT (synthetic weights), K = 1, 2, 4, 8 stream=True utterances at the
# facade's 50-frame hop, all K at a depth of 10 s (500 frames) or 32 s (1600 frames) of mel.  Per poll, two forms on the same mels:
#   batched - ONE HiftEngine.inference_streams call over K slots of one handle (fy_hift_infer_streams);
#   serial  - K single-stream incremental calls (FY_INCREMENTAL) one after another on K handles: what tts_stream_batch did before
#             the vocoder had stream slots, and the yardstick.
# Each poll is timed with HIP events on the calls' stream (output allocation and the mel slices' copies included, as in the facade);
# the polls are consecutive hops from the depth on (an incremental call's window is 95 frames whatever the depth), the two forms
# alternate poll by poll, and the median of the polls after the warm-up is taken.  Every (K, depth) step - and the step that
# weighs a 3200-frame handle against a slot session - runs in a fresh child process under its own time limit; the first step that
# fails ends the run.
#   python tests/micro/hift_stream_slots_probe.py [--polls 12] [--out FILE.json]   (default: profiles/hift_stream_slots_probe.json)
import argparse, json, os, statistics, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--polls", type=int, default=12)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hift_stream_slots_probe.json"))
ap.add_argument("--step", nargs=2, type=int, metavar=("K", "DEPTH"), help="(child) one measurement; prints a JSON line")
ap.add_argument("--bytes", action="store_true", help="(child) device bytes of a 3200-frame handle and of an 8-slot session")
ap.add_argument("--step-timeout", type=int, default=240)
args = ap.parse_args()
UP, HOP = 480, 50


def child_setup():
    import torch
    sys.path.insert(0, ROOT)
    from fangyan_tts_amd import synth
    from fangyan_tts_amd.hift import HiftEngine
    from fangyan_tts_amd.spec import HiftCfg
    dev = torch.device("cuda:0")
    cfg = HiftCfg()
    return torch, synth, HiftEngine, cfg, dev, synth.state_dict_torch(cfg.manifest(), dev)


def step(K, depth):
    torch, synth, HiftEngine, cfg, dev, sd = child_setup()
    n_polls = args.warmup + args.polls
    total = depth + HOP * n_polls
    one = HiftEngine(sd, cfg, max_batch=K, max_frames=total, device=dev)
    many = [HiftEngine(sd, cfg, max_batch=1, max_frames=total, device=dev) for _ in range(K)]
    mels = [torch.rand(1, 80, total, generator=torch.Generator(device="cpu").manual_seed(100 + i)).to(dev) for i in range(K)]
    ri = torch.from_numpy(synth.hift_rand_ini()).to(dev)
    sn = torch.from_numpy(synth.hift_sine_noise(total * UP)).to(dev)
    st = torch.cuda.current_stream(dev)
    slots = list(range(K))

    def batched(F):
        return one.inference_streams(slots, [m[:, :, :F] for m in mels], ri, sn, [False] * K)

    def serial(F):
        return [e.inference(m[:, :, :F].contiguous(), ri, sn, finalize=False, incremental=True)[0] for e, m in zip(many, mels)]

    one.open_streams(K)
    for e in many:
        e.stream_reset()
    batched(depth - HOP)                                        # every stream to the depth: the polls below bring HOP frames each
    got = serial(depth - HOP)
    torch.cuda.synchronize()
    ms = {"batched": [], "serial": []}
    same = True
    for p in range(n_polls):
        F = depth + HOP * p
        order = (("batched", batched), ("serial", serial)) if p % 2 == 0 else (("serial", serial), ("batched", batched))
        out, evs = {}, {}
        for name, fn in order:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st)
            out[name] = fn(F)
            b.record(st)
            evs[name] = (a, b)
        torch.cuda.synchronize()
        lo, hi = UP * (F - HOP - 8), UP * (F - 8)
        same = same and all(torch.equal(x, y[0, lo:hi]) for x, y in zip(out["batched"], out["serial"]))
        if p >= args.warmup:
            for name, (a, b) in evs.items():
                ms[name].append(a.elapsed_time(b))
    window = one.stream_slot_window(0)
    one.close_streams()
    r = {"K": K, "depth_frames": depth, "polls": args.polls, "window": window, "identical": same,
         "ms_batched": round(statistics.median(ms["batched"]), 4), "ms_serial": round(statistics.median(ms["serial"]), 4),
         "ms_batched_min_max": [round(min(ms["batched"]), 4), round(max(ms["batched"]), 4)],
         "ms_serial_min_max": [round(min(ms["serial"]), 4), round(max(ms["serial"]), 4)]}
    print("RESULT " + json.dumps(r), flush=True)


def weigh():
    torch, synth, HiftEngine, cfg, dev, sd = child_setup()
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info(dev)
    e = HiftEngine(sd, cfg, max_batch=1, max_frames=3200, device=dev)
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info(dev)
    big = HiftEngine(sd, cfg, max_batch=8, max_frames=64, device=dev)
    big.open_streams(8)
    r = {"handle_3200_frames_bytes": int(free0 - free1), "session_8_slots_bytes": big.streams_bytes()}
    big.close_streams()
    del e
    print("RESULT " + json.dumps(r), flush=True)


def run_child(extra):
    cmd = [sys.executable, os.path.abspath(__file__), "--polls", str(args.polls), "--warmup", str(args.warmup)] + extra
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f"step {extra} ended with status {p.returncode}: nothing more is started")
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


if args.step:
    step(*args.step)
elif args.bytes:
    weigh()
else:
    rec = {"config": "HiftCfg() full size, synthetic weights; ms per poll (K streams, 50 new frames each) by HIP events, median over the polls; "
                     "batched = one fy_hift_infer_streams call, serial = K single-stream FY_INCREMENTAL calls on K handles",
           "memory": run_child(["--bytes"]), "steps": []}
    print(rec["memory"], flush=True)
    for depth in (500, 1600):
        for K in (1, 2, 4, 8):
            r = run_child(["--step", str(K), str(depth)])
            rec["steps"].append(r)
            print(f"K {K} depth {depth}: batched {r['ms_batched']:.3f} ms, serial {r['ms_serial']:.3f} ms per poll "
                  f"(window {r['window']}, identical {r['identical']})", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(rec, open(args.out, "w"), indent=1)
    print("wrote", args.out)
