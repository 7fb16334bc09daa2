"""The float64 reference, the error bounds, the inputs and the case lists of the direct DiT attention tests
(tests/test_attention_ref_cpu.py proves on the CPU that the cases can fail; tests/test_attention_gpu.py runs the kernels).

Operation (per sequence and head, head dimension 64): scores q k^T * 0.125; key j is visible to query i iff j < len, and
j < (i // chunk + 1) * chunk when chunk > 0; o = softmax(scores) v.  The reference works in torch float64 on the exact values
the kernel receives (bf16, or hi + lo of the split planes) and also returns a = sum_j p_ij |v_jd|, the scale of the
numerator's rounding error.

Bound of the bf16 kernels, per output element: |got - o| <= 2^-8 (|o| + a) + 1e-6.  The probabilities are rounded to bf16
(relative error <= 2^-9: a numerator error <= 2^-9 a); the denominator sums the same probabilities, or the fp32 ones
(<= 2^-9 relative on o); the output is rounded to bf16 (2^-9 |o|); fp32 accumulation and the hardware exp2 are orders
smaller.  Bound of the split (hi + lo) kernels: 2^-14 (|o| + a) at query scale <= 3 - the dropped lo x lo terms and the hi / lo
splits of p and of the output are 2^-16-class each.  Neither is tuned on a kernel: `emulate` (NumPy, fp32, probabilities
rounded to bf16 tile by tile) has to stay inside the first, and a mask that is off by one key has to leave both by a factor.
"""
import functools
from collections import namedtuple

import numpy as np
import torch

from fangyan_tts_amd import synth
from fangyan_tts_amd.spec import FlowCfg

D = 64
CHUNK = FlowCfg().static_chunk
LOG2E = 1.4426950408889634


# ---- reference -------------------------------------------------------------------------------------------------------------
def visible(n, chunk, len_shift=0, lim_shift=0):
    """bool [n][n]: key j visible to query i.  The shifts move the sequence end / the chunk limit (the CPU test's mutants)."""
    i = torch.arange(n)[:, None]
    j = torch.arange(n)[None, :]
    m = j < n + len_shift
    if chunk > 0:
        m = m & (j < (i // chunk + 1) * chunk + lim_shift)
    return m.expand(n, n)


def ref(q, k, v, n, chunk, mask=None):
    """q, k, v: [T >= n][H][64] (any float dtype); returns float64 o, a of shape [n][H][64]."""
    q, k, v = (x[:n].double().permute(1, 0, 2) for x in (q, k, v))                   # [H][n][64]
    s = q @ k.transpose(1, 2) * 0.125
    s = s.masked_fill(~(visible(n, chunk) if mask is None else mask), float("-inf"))
    p = torch.softmax(s, dim=-1)
    return (p @ v).permute(1, 0, 2).contiguous(), (p @ v.abs()).permute(1, 0, 2).contiguous()


def ref_batch(X, lens, chunk, **shifts):
    """X: [nseq][Tmax][3][H][64]; a list of (o, a) per sequence."""
    return [ref(X[s, :, 0], X[s, :, 1], X[s, :, 2], n, chunk, visible(n, chunk, **shifts) if shifts else None) for s, n in enumerate(lens)]


def bound_bf16(o, a):
    return 2.0 ** -8 * (o.abs() + a) + 1e-6


def bound_split(o, a):
    return 2.0 ** -14 * (o.abs() + a)


def ratio(got, o, bound):
    """The largest |got - o| / bound over the elements."""
    return float(((got.double() - o).abs() / bound).max())


def emulate(q, k, v, n, chunk, tile, sum_bf16):
    """NumPy fp32 emulation of the bf16 kernels' rounding: online softmax over `tile` keys at a time in the exp2 domain, the
    probabilities rounded to bf16 before the second product, the denominator over the rounded (sum_bf16: the round-5 kernel's
    ones-MFMA) or the fp32 probabilities (round 2), the output rounded to bf16.  [n][H][64] float32."""
    r = synth.bf16_round
    q, k, v = (np.ascontiguousarray(x[:n].float().numpy().transpose(1, 0, 2)) for x in (q, k, v))
    H = q.shape[0]
    s = (q @ k.transpose(0, 2, 1)).astype(np.float32) * np.float32(0.125 * LOG2E)
    s = np.where(visible(n, chunk).numpy()[None], s, np.float32(-1e30))
    m = np.full((H, n, 1), -1e30, np.float32)
    l = np.zeros((H, n, 1), np.float32)
    o = np.zeros((H, n, D), np.float32)
    for k0 in range(0, n, tile):
        st = s[:, :, k0:k0 + tile]
        mn = np.maximum(m, st.max(axis=2, keepdims=True))
        alpha = np.exp2(m - mn)
        p = np.where(st > -1e29, np.exp2(st - mn), np.float32(0)).astype(np.float32)
        pb = r(p)
        l = l * alpha + (pb if sum_bf16 else p).sum(axis=2, keepdims=True, dtype=np.float32)
        o = o * alpha + pb @ v[:, k0:k0 + tile]
        m = mn
    return torch.from_numpy(r((o / l).astype(np.float32)).transpose(1, 0, 2).copy())


# ---- inputs ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pool(name, H):
    """Normal draws [nseq][T][H][64], one pool per head count (every case is a slice of it)."""
    return torch.from_numpy(synth.normal(f"in.attn.{name}.{H}", (8, 650, H, D) if H <= 2 else (4, 65, H, D)))


def _bf16(x):
    return x.to(torch.bfloat16).float()


_U = torch.tensor([(1.0 if (d * (d + 1) // 2) % 3 else -1.0) / 8.0 for d in range(D)])       # a fixed unit vector


def inputs(lens, mode="default", H=2):
    """[nseq][Tmax][3][H][64] float32 holding bf16-representable values: q = scale * draws, k, v = draws.
    rising / falling: k += +-0.25 j u and q += 16 u for the unit vector u, so the score of key j moves by about +-0.5 j for
    every query (q.u has deviation 3): the running maximum moves in every tile / never after the first.  flat: q = 0, the
    output is the mean of the visible v rows.  hot: query scale 8, most probabilities underflow bf16."""
    nseq, T = len(lens), max(lens)
    q, k, v = (_pool(n, H)[:nseq, :T].clone() for n in "qkv")
    q *= {"flat": 0.0, "hot": 8.0}.get(mode, 3.0)
    if mode in ("rising", "falling"):
        j = torch.arange(T, dtype=torch.float32)[None, :, None, None]
        k += (0.25 if mode == "rising" else -0.25) * j * _U
        q += 16.0 * _U
    return _bf16(torch.stack([q, k, v], dim=2))


def inputs_split(lens, H=2):
    """The split kernels' operands: fp32 x (query scale 3), hi = bf16(x), lo = bf16(x - hi).  Returns (hi, lo)."""
    nseq, T = len(lens), max(lens)
    q, k, v = (_pool(n, H)[:nseq, :T].clone() for n in "qkv")
    x = torch.stack([3.0 * q, k, v], dim=2)
    hi = _bf16(x)
    return hi, _bf16(x - hi)


# ---- cases -----------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "lens chunk mode H")


def cid(c):
    return f"{'.'.join(map(str, c.lens))}-c{c.chunk}-{c.mode}" + (f"-H{c.H}" if c.H != 2 else "")


RAGGED = [[1, 31, 32, 33, 63, 64, 65, 96], [97, 127, 128, 129, 255, 256, 257, 2]]
# the round-5 dispatch's edges: 256 / 257 (four to eight waves), 400, 512 / 513 (eight back to four), 650
EDGES = [[256, 255, 225, 256, 31, 256, 193, 2], [257, 256, 225, 257, 31, 257, 193, 2], [400, 377, 400, 256, 400, 129, 31, 390],
         [512, 449, 448, 512, 65, 512, 500, 1], [513, 512, 481, 513, 257, 513, 33, 7], [650, 611, 333, 650, 1, 650, 640, 97]]
CHUNKS = [0, CHUNK, 32, 64, 7]            # 7: the limit arithmetic must not assume a multiple of the 32-key half tile

DIRECT = [Case(l, c, "default", 2) for l in RAGGED for c in CHUNKS]
DIRECT += [Case(l, c, "default", 2) for l in EDGES for c in (0, CHUNK, 7)]
DIRECT += [Case(l, c, "default", 2) for l in (EDGES[2], EDGES[5]) for c in (32, 64)]
DIRECT += [Case(l, c, m, 2) for l in RAGGED + [EDGES[5]] for m in ("rising", "flat", "hot") for c in (0, CHUNK, 7)]
# falling: the edge keys are the lightest there - only a sequence of two frames and the 7-frame chunks keep an off-by-one mask visible
DIRECT += [Case(l, c, "falling", 2) for l in ([2, 31, 32, 33, 63, 64, 65, 96], RAGGED[1], [650, 611, 333, 650, 2, 650, 640, 97]) for c in (0, 7)]
DIRECT += [Case([65, 64, 1, 33], CHUNK, "default", 16)]

# q_begin > 0 (incremental chunks): (lens, chunk, interleaved); interleaved with two sequences is the flow decoder's incremental call
QBEGIN = [(l, c, il) for l in ([300, 300], [150, 131], [300, 287, 150, 33]) for c in (CHUNK, 7) for il in (False, True)]


def q_begins(lens, chunk):
    return sorted({32, chunk, 100, max(lens) - 1})


# the per-sequence table forms: (name, row_step, [(q_begin, len)] per sequence).  row_step 2: sequences 2 i, 2 i + 1 are slot i's
# interleaved pair (in_row = 2 cap i + s); row_step 1: disjoint blocks.  With a sequence that has no query and one of length 1.
TAB = [("slots", 2, [(100, 150), (100, 150), (64, 64), (0, 1)]),
       ("slots-long", 2, [(250, 300), (250, 300), (0, 57), (7, 57)]),
       ("blocks", 1, [(32, 97), (0, 33), (129, 129), (0, 1)])]
TAB_CHUNKS = [CHUNK, 7, 0]

SPLIT_LENS = [[33, 32, 31, 1], [129, 128, 97, 65, 2], [161, 160, 129, 64], [193, 191, 33], [225, 224, 193, 7], RAGGED[1], EDGES[4]]
SPLIT = [Case(l, c, "split", 2) for l in SPLIT_LENS for c in (0, CHUNK, 7)]
# split_tab against split: the slots' layout, and the single stream's incremental call (q_begin = T0, two interleaved sequences)
SPLIT_TAB = [("slots", 2, [(100, 150), (100, 150), (64, 64), (0, 1)]), ("incremental", 2, [(200, 250), (200, 250)]),
             ("incremental-long", 2, [(250, 300), (250, 300)])]
