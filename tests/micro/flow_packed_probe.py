# Packed rows (FY_PACKED): what a ragged flow batch costs padded and packed, on the same handle in the same process.  Full size,
# batch 8 against a 400-frame maximum, (a) uniform lengths - equal row counts: what the extra small launches cost, (b) lengths
# spread evenly over 0.5 - 1.0 of the maximum, (c) a streaming final group of 3 with one sequence a tenth as long as the others;
# each in the default arithmetic and with FY_PRECISE.  HIP-event time per call; after two warm calls of each leg, the median of
# REPS calls, the two legs alternated so that clock and cache state drift hits both alike.  (a) forces the packed path onto a
# uniform batch by shortening one utterance by one token (2 rows of 6400).  No threshold: the record is the result.
# Writes profiles/flow_packed_probe.json.   timeout 600 python tests/micro/flow_packed_probe.py
import json, os, statistics, sys, torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from fangyan_tts_amd import _lib, synth
from fangyan_tts_amd.flow import FlowEngine, packed_rows
from fangyan_tts_amd.spec import FlowCfg
cfg = FlowCfg(); dev = torch.device("cuda:0")
TMAX, B, REPS = 400, 8, 7
sd = synth.state_dict_torch(cfg.manifest(), dev)
eng = FlowEngine(sd, cfg, max_batch=B, max_frames=TMAX, device=dev)
noise = torch.from_numpy(synth.flow_rand_noise(TMAX)).to(dev)

def batch(n_tok):
    b = len(n_tok)
    return (torch.from_numpy(synth.randint("probe.packed.tok", (b, max(n_tok)), 0, cfg.vocab)).to(dev), n_tok, torch.zeros(b, 1, dtype=torch.int32, device=dev), [0] * b,
            torch.zeros(b, 1, 80, device=dev), [0] * b, torch.from_numpy(synth.normal("probe.packed.spk", (b, cfg.spk_in))).to(dev), noise)

def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); a.record(); fn(); b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b)

N = TMAX // 2
cases = {"a_uniform": [N] * (B - 1) + [N - 1],
         "b_spread_half_to_full": [round(N * (0.5 + 0.5 * i / (B - 1))) for i in range(B)],
         "c_final_group_of_3": [N, N // 10, N]}
res = {"config": {"frames_max": TMAX, "batch": B, "reps": REPS, "ln_fold": eng.ln_fold, "weight_planes": eng.weight_planes}, "cases": {}}
for name, n_tok in cases.items():
    args = batch(n_tok)
    T = [2 * n for n in n_tok]
    for arith, flags in (("default", 0), ("precise", _lib.FY_PRECISE)):
        legs = {"padded": lambda: eng.inference(*args, flags=flags), "packed": lambda: eng.inference(*args, flags=flags, packed=True)}
        rows, ms = {}, {k: [] for k in legs}
        for k, fn in legs.items():
            fn(); fn()
            rows[k] = eng.last_rows
        for _ in range(REPS):
            for k, fn in legs.items():
                ms[k].append(timed(fn))
        assert rows["padded"] == 2 * len(T) * max(T) and rows["packed"] == packed_rows(T)[1], rows
        med = {k: statistics.median(v) for k, v in ms.items()}
        row = {"n_token": n_tok, "rows_padded": rows["padded"], "rows_packed": rows["packed"], "rows_ratio": round(rows["packed"] / rows["padded"], 4),
               "ms_padded_median": round(med["padded"], 3), "ms_packed_median": round(med["packed"], 3),
               "ms_padded_min_max": [round(min(ms["padded"]), 3), round(max(ms["padded"]), 3)],
               "ms_packed_min_max": [round(min(ms["packed"]), 3), round(max(ms["packed"]), 3)],
               "time_ratio_packed_over_padded": round(med["packed"] / med["padded"], 4)}
        res["cases"][f"{name}.{arith}"] = row
        print(name, arith, json.dumps(row), flush=True)
res["note"] = ("the rotary embedding stays in the qkv product's epilogue (a table with one row per compact row): no separate rotate-and-store launch; "
               "a packed call adds one table upload and one table launch per call and one gather launch per Euler step")
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
json.dump(res, open(os.path.join(ROOT, "profiles", "flow_packed_probe.json"), "w"), indent=1)
