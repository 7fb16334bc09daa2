"""The float64 references, the error bounds, the inputs and the case lists of the direct tests of the speech-token LM's decode
products (gemv_bf16w, gemv32, gv32_split_rows) and cache attention (llm_attention, llm_attention_step).
tests/test_llm_ref_cpu.py proves on the CPU that the cases can fail; tests/test_llm_kernels_gpu.py runs the kernels.  Nothing in
here comes from a kernel: layouts are written from the text of gemm.h / gemv32.h, bounds from the arithmetic below (u = 2^-24).

Linear products, exact inputs.  x = 2 i0 + i1 2^-8 + i2 2^-16 with i* in {-1, 1} on a sparse support (0 elsewhere) and
W in {-1, 0, 1} 2^e.  (The leading digit is 2, not 1: with |x| < 2 the residual x - bf16(x) is a multiple of 2^-16 below 2^-8,
which always fits ONE bf16, and the lo plane would be empty.  With i0 = i1 = i2 the value lies above 2, hi is 2 i0 and the residual i1 (2^-8 + 2^-16) needs nine
bits: a quarter of the support has all three planes - where i1 differs from i0 the value lies below 2, hi is 2 - 2^-7 and one
bf16 holds the rest.  The CPU test shows that this is enough for every row and tile.)  The builder asserts max |x| |W|^T < 2^(8 + e): every product
and every partial sum, in any order, is then a multiple of 2^(e - 16) below 2^(8 + e) - 24 bits - so fp32 summation is exact in
every order and the kernel must return the float64 result bit for bit.  Residuals and biases are multiples of 2^(e - 16) below
2^(e + 4), so y + Wx and Wx + b stay exact.  Two weight planes: W = (w0 + w1 2^-9) 2^e, whose bf16 split is w0 (or w1 2^-9 where
w0 = 0) plus the rest, against an x = 2 i0 + i1 2^-8 whose lo plane is empty: the one term the kernel drops, lo x lo, is zero,
and every product is a multiple of 2^(e - 17) below 2^(7 + e) (the builder asserts that tighter limit there).

Linear products, random inputs.  W bf16-representable, x normal with a wide per-row range: the three-plane split is exact, the
products are exact, K of them are summed in fp32 in some order: |got - ref| <= K u S + 1e-30, S = |x| |W|^T (the bound of
test_exact_split_products_ring_and_register_staged).  Two weight planes: + u S for the dropped lo x lo term (2^-26 of a product
per term by gemv32.h, bounded generously).

Fused RMSNorm: ref = rsqrt(mean(x^2) + eps) (W (norm_w x)).  With exact inputs (norm_w a power of two) the product is exact; the
sum of squares rounds each square (u / 2) and adds K terms ((K - 1) u in any order): <= K u relative, K u / 2 on its inverse root;
the division by K, the + eps, rsqrtf (<= 2 u) and the multiply add <= 4 u: (K / 2 + 8) u relative.  Random inputs add the product
bound with one more rounding per term (norm_w x is rounded before the split).

SwiGLU: act_silu(g) = g / (1 + expf(-g)): expf <= 1 ulp = 2 u, it enters 1 + e with weight e / (1 + e) < 1; the sum rounds (u), the
division (<= 2 u) and the multiply by `up` (u): <= 6 u < 2^-20 relative, on exact g and up.  Random inputs add the first-order
effect of the product errors (|silu'| <= 1.1).

Attention (fp32, head dim 64, scale 0.125, row r sees keys 0..row_pos[r] of sequence row_seq[r]).  The step form rotates q and
the new k by the split-half RoPE at the fp32 angle float32(pos) * inv_freq[d & 31]; the reference takes float64 sin / cos of that
fp32 number.  A rotated element is two products and a sum with a <= 2 ulp sin / cos: <= 4 ulp = 8 u of |x cos| + |x' sin| (the
cache-row check).  Score: a 64-term fma chain, <= 64 u A_j with A_j = 0.125 sum_d |q_d| |k_jd| (+ 16 u A_j in the step form for
the two rotations); the subtraction of the maximum rounds by <= u |s_j - max|; expf <= 2 u; so the probability of key j has a
relative error <= e_j = u ((64 + rot) A_j + |s_j - max| + 4), each key by its OWN A_j (a common factor cancels in the quotient).
The n-term fma sums of numerator and denominator add n u each, the new key's product and the division 2 u:
    |got - o| <= (n + 4) u (|o| + a) + sum_j p_j e_j |v_jd| + |o| sum_j p_j e_j + 1e-30,   a = sum_j p_j |v_jd|,
i.e. c(n) = n + 4 + (the p-weighted mean of e_j) / u.  The NumPy fp32 emulation of the CPU test has to stay inside it.
"""
import functools
from collections import namedtuple

import numpy as np

from fangyan_tts_amd import synth

U = 2.0 ** -24
GV_STORE, GV_ADD, GV_SWIGLU, GV_SWIGLU_SPLIT = 0, 1, 2, 3
GV32_STORE, GV32_ADD_IMG, GV32_SWIGLU_IMG = 0, 1, 2
EPS = 1e-6


# ---- the three-way split and the layouts (gemm.h, gemv32.h) -------------------------------------------------------------------
def split3(x):
    """fp32 -> (hi, mid, lo) fp32 arrays holding bf16 values: hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid)."""
    x = np.asarray(x, np.float32)
    hi = synth.bf16_round(x)
    r1 = (x - hi).astype(np.float32)
    mid = synth.bf16_round(r1)
    lo = synth.bf16_round((r1 - mid).astype(np.float32))
    return hi, mid, lo


def bits(x):
    """bf16-representable fp32 -> uint16 bit patterns"""
    return (np.ascontiguousarray(x, np.float32).view(np.uint32) >> np.uint32(16)).astype(np.uint16)


def unbits(b):
    return (np.asarray(b, np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def image_encode(planes):
    """planes [3][R][K] fp32 (bf16 values) -> uint16 [ceil(R/32)][K/16][3][64][8]: lane l of fragment kk holds row l & 31,
    columns 16 kk + 8 (l >> 5) .. + 7; rows beyond R are zero."""
    _, R, K = planes.shape
    Z = (R + 31) // 32
    p = np.zeros((3, Z * 32, K), np.uint16)
    p[:, :R] = bits(planes)
    p = p.reshape(3, Z, 32, K // 16, 2, 8)                     # plane, slice, row, fragment, half, j
    return np.ascontiguousarray(p.transpose(1, 3, 0, 4, 2, 5)).reshape(Z, K // 16, 3, 64, 8)


def image_decode(img, R, K):
    """uint16 image -> fp32 [3][32 ceil(R/32)][K] (every row of the slices, so that the padding can be checked)"""
    Z = (R + 31) // 32
    p = np.asarray(img, np.uint16).reshape(Z, K // 16, 3, 2, 32, 8).transpose(2, 0, 4, 1, 3, 5)
    return unbits(np.ascontiguousarray(p).reshape(3, Z * 32, K))


def image_of(x):
    """fp32 [R][K] -> the image of its exact split"""
    return image_encode(np.stack(split3(x)))


def planes8_encode(x, ld):
    """fp32 [R][K] -> uint16 [ceil(R/8)][24][ld], the pre-split operand of gemv_bf16w: rows 0-7 hi, 8-15 mid, 16-23 lo of
    each group of 8 rows (zero elsewhere)."""
    R, K = x.shape
    Z = (R + 7) // 8
    out = np.zeros((Z, 3, 8, ld), np.uint16)
    for p, pl in enumerate(split3(x)):
        b = np.zeros((Z * 8, K), np.uint16)
        b[:R] = bits(pl)
        out[:, p, :, :K] = b.reshape(Z, 8, K)
    return out.reshape(Z, 24, ld)


def planes8_decode(buf, R, N):
    """uint16 [ceil(R/8)][24][ld] -> fp32 [3][R][N]"""
    Z = (R + 7) // 8
    b = np.asarray(buf, np.uint16).reshape(Z, 3, 8, -1)[..., :N]
    return unbits(np.ascontiguousarray(b.transpose(1, 0, 2, 3)).reshape(3, Z * 8, N)[:, :R])


# ---- inputs of the products ----------------------------------------------------------------------------------------------------
RMAX = 40


def _signs(name, shape):
    return np.where(synth.uniform(name, shape, 0.0, 1.0) < 0.5, -1.0, 1.0)


def _density(K, planes_w):
    """of the supports of x and W: the mean of |x| |W|^T is 2 K d^2 = 64 (32 with two weight planes, whose limit is 2^7)"""
    return min(0.5, ((32.0 if planes_w == 1 else 16.0) / K) ** 0.5)


@functools.lru_cache(maxsize=None)
def exact_inputs(N, K, e=0, planes_w=1, rows=RMAX, small=False):
    """x [rows][K], W [N][K], W_lo ([N][K] or None; W + W_lo is the matrix), bias [N], resid [rows][N], norm_w [K], all float64
    arrays of fp32-representable values as the module docstring describes them.  small: the rows of x times 2^-10 (the fused
    norm's eps then matters; a power of two keeps everything exact, limits 2^-10 lower)."""
    tag = f"in.llmk.exact.{N}.{K}.{e}.{planes_w}"
    d = _density(K, planes_w)
    sup = synth.uniform(tag + ".xs", (rows, K), 0.0, 1.0) < d
    x = 2.0 * _signs(tag + ".x0", (rows, K)) + _signs(tag + ".x1", (rows, K)) * 2.0 ** -8
    if planes_w == 1:
        x = x + _signs(tag + ".x2", (rows, K)) * 2.0 ** -16
    x = np.where(sup, x, 0.0)
    w0 = np.where(synth.uniform(tag + ".ws", (N, K), 0.0, 1.0) < d, _signs(tag + ".w0", (N, K)), 0.0)
    W, W_lo = w0 * 2.0 ** e, None
    if planes_w == 2:
        full = (w0 + np.where(synth.uniform(tag + ".w1s", (N, K), 0.0, 1.0) < d, _signs(tag + ".w1", (N, K)), 0.0) * 2.0 ** -9) * 2.0 ** e
        W = synth.bf16_round(full.astype(np.float32)).astype(np.float64)
        W_lo = full - W
        assert np.array_equal(synth.bf16_round(W_lo.astype(np.float32)).astype(np.float64), W_lo)
        assert not np.stack(split3(x.astype(np.float32)))[2].any()                   # lo x lo, the dropped term, is zero
    norm_w = 2.0 ** np.floor(synth.uniform(tag + ".nw", (K,), 0.0, 2.0)) * _signs(tag + ".nws", (K,))    # +-1, +-2
    # the limit leaves room for a bias and a residual below 2^(e + 3) each, and holds with the fused norm's weight applied
    S = np.abs(x * (norm_w if planes_w == 1 else 1.0)) @ (np.abs(W) + (0 if W_lo is None else np.abs(W_lo))).T
    assert S.max() + 2.0 ** (e + 4) < 2.0 ** (8 + e - (1 if planes_w == 2 else 0)), S.max()
    q = 2.0 ** (e - 16)
    bias = np.round(synth.uniform(tag + ".b", (N,), -2.0 ** 19, 2.0 ** 19)) * q
    resid = np.round(synth.uniform(tag + ".r", (rows, N), -2.0 ** 19, 2.0 ** 19)) * q
    if small:
        x, resid, bias = x * 2.0 ** -10, resid * 2.0 ** -10, bias * 2.0 ** -10
    for a in (x, W, bias, resid, norm_w):
        assert np.array_equal(a.astype(np.float32).astype(np.float64), a)
    return x, W, W_lo, bias, resid, norm_w


@functools.lru_cache(maxsize=None)
def random_inputs(N, K, planes_w=1, rows=RMAX):
    """x normal with a per-row scale exp(3 z) (a wide dynamic range), W bf16-representable (two planes: W + W_lo with both
    bf16), bias / resid / norm_w normal; float64 arrays of fp32 values."""
    tag = f"in.llmk.rand.{N}.{K}.{planes_w}"
    x = synth.normal(tag + ".x", (rows, K)) * np.exp(3.0 * synth.normal(tag + ".xs", (rows, 1))).astype(np.float32)
    w = synth.normal(tag + ".w", (N, K))
    W, W_lo = synth.bf16_round(w), None
    if planes_w == 2:
        W_lo = synth.bf16_round((w - W).astype(np.float32))
    f = lambda a: None if a is None else a.astype(np.float32).astype(np.float64)
    return (f(x), f(W), f(W_lo), f(synth.normal(tag + ".b", (N,))), f(synth.normal(tag + ".r", (rows, N))),
            f(synth.normal(tag + ".nw", (K,), 1.0, 0.25)))


# ---- references and bounds of the products -------------------------------------------------------------------------------------
Prod = namedtuple("Prod", "y bound g u rstd")


def silu(g):
    return g / (1.0 + np.exp(-g))


def product_ref(x, W, W_lo=None, bias=None, resid=None, norm_w=None, eps=EPS, swiglu=False, exact=False, rstd=None):
    """float64 reference and bound of one product call.  x [R][K]; resid: y += (GV_ADD / GV32_ADD_IMG); norm_w: the fused
    RMSNorm computed here from x; rstd [R]: a given 1/rms instead (gemv32: the image already holds norm_w x); swiglu: the rows
    of W are (gate_i, up_i) interleaved, y [R][N/2].  exact: the inputs are exact_inputs' (the product itself carries no error)."""
    K = x.shape[1]
    Wt = W if W_lo is None else W + W_lo
    xn = x if norm_w is None else (x.astype(np.float32) * norm_w.astype(np.float32)).astype(np.float64)
    if norm_w is not None and exact:
        assert np.array_equal(xn, x * norm_w)
    p = xn @ Wt.T
    S = np.abs(xn) @ np.abs(Wt).T
    bp = np.zeros_like(p) if exact else (K + (1 if norm_w is not None else 0) + (1 if W_lo is not None else 0)) * U * S
    if norm_w is not None and rstd is None:
        rstd = 1.0 / np.sqrt((x * x).mean(axis=1) + eps)
    if rstd is not None:
        p, bp = p * rstd[:, None], bp * rstd[:, None] + (K / 2 + 8) * U * np.abs(p * rstd[:, None])
    y = p
    if bias is not None:
        y = y + bias
        # the one rounding of the sum: up to u |y| by itself, so where the product is small beside the bias a correct kernel
        # sits at 0.5 to 1.0 of this bound - that is the rounding, not a reason to widen it
        if not (exact and rstd is None):
            bp = bp + U * np.abs(y)
    g = u = None
    if swiglu:
        g, u = y[:, 0::2], y[:, 1::2]
        bg, bu = bp[:, 0::2], bp[:, 1::2]
        y = silu(g) * u
        bp = 1.1 * bg * np.abs(u) + np.abs(silu(g)) * bu + 1.1 * bg * bu + 2.0 ** -20 * np.abs(y)
    if resid is not None:
        y = resid + y
        if not (exact and rstd is None):
            bp = bp + U * np.abs(y)
    return Prod(y, bp + 1e-30, g, u, rstd)


def ratio(got, ref, bound):
    return float((np.abs(np.asarray(got, np.float64) - ref) / bound).max())


def ssq_ref(x):
    """per-32-column sums of x^2: [K/32][R] float64"""
    R, K = x.shape
    return (x * x).reshape(R, K // 32, 32).sum(axis=2).T


# bf16 ends at 2^-133: three planes hold all 24 bits of an fp32 value only from 2^-109 on (a SwiGLU output under a gate of -80
# lies below that; its planes then only have to add up to a value inside the bound)
SPLIT_EXACT_FROM = 2.0 ** -109
SSQ_REL = 40 * U                                   # 32 squares (u / 2 each) summed in some order (31 u), with slack


# ---- product cases -------------------------------------------------------------------------------------------------------------
R8 = (1, 7, 8, 9, 20)
STAGED8 = [(64, 128), (896, 896), (101, 1024), (6761, 896)]           # (N, K) of the LDS-staged form (K <= 1024, K % 128 == 0)
# the pre-split form: (N, K, workspace).  K/16 = 304 fragments in 4 slices of 76; 129 in 33 / 33 / 33 / 30; 133 in one slice:
# two trips of the 128-fragment loop
DIRECT8 = [(896, 4864, True), (64, 2064, True), (64, 2128, False)]
R32 = (1, 9, 31, 32, 33, 40)
# (name, N, K, workspace): one per launch form of gemv32 at the default thresholds
FORMS32 = [("1x8", 896, 896, False), ("1x4", 4128, 128, False), ("2x4", 8224, 128, False), ("splitk", 896, 4864, True),
           ("splitk-uneven", 64, 2064, True), ("store-ragged", 6761, 896, False)]
XW32 = [("1x8", 896, 896), ("1x4", 4128, 128), ("2x4", 8224, 128)]


# ---- attention -----------------------------------------------------------------------------------------------------------------
D = 64
SCALE = 0.125


def inv_freq(theta=1e6):
    return (1.0 / theta ** (np.arange(32, dtype=np.float64) / 32.0)).astype(np.float32)


def rope(x, pos, invf):
    """split-half rotation of x [..., 64] (float64) at the fp32 angle float32(pos) * invf[d & 31]; also returns the magnitude
    |x cos| + |x' sin| of each element (the scale of its rounding error)."""
    ang = (np.float32(pos) * invf.astype(np.float32)).astype(np.float32).astype(np.float64)
    c, s = np.cos(ang), np.sin(ang)
    a, b = x[..., :32], x[..., 32:]
    out = np.concatenate([a * c - b * s, b * c + a * s], axis=-1)
    mag = np.concatenate([np.abs(a * c) + np.abs(b * s), np.abs(b * c) + np.abs(a * s)], axis=-1)
    return out, mag


def attend(q, keys, vals, rot):
    """q [64], keys / vals [n][64] float64 -> o [64], bound [64] (module docstring)"""
    n = keys.shape[0]
    s = SCALE * (keys @ q)
    A = SCALE * (np.abs(keys) @ np.abs(q))
    p = np.exp(s - s.max())
    p /= p.sum()
    o, a = p @ vals, p @ np.abs(vals)
    e = U * ((64 + rot) * A + (s.max() - s) + 4)
    return o, (n + 4) * U * (np.abs(o) + a) + (p * e) @ np.abs(vals) + np.abs(o) * (p @ e) + 1e-30


def attention_ref(q, Kc, Vc, row_seq, row_pos, Hq, Hk, mutant=None):
    """llm_attention.  q [R][Hq 64], Kc / Vc [seq][Hk][ctx][64] (float64).  Returns o, bound [R][Hq 64] (NaN rows where the
    mutant is undefined).  mutant: drop_last | stale | seq0 | group."""
    R = q.shape[0]
    o, b = np.full((R, Hq * D), np.nan), np.full((R, Hq * D), np.nan)
    grp = Hq // Hk
    for r in range(R):
        seq, n = (0 if mutant == "seq0" else row_seq[r]), row_pos[r] + 1
        if mutant == "drop_last":
            n -= 1
        if mutant == "stale":
            n += 1
        if n < 1 or n > Kc.shape[2]:
            continue
        for h in range(Hq):
            hk = (h // grp + (1 if mutant == "group" else 0)) % Hk
            o[r, h * D:(h + 1) * D], b[r, h * D:(h + 1) * D] = attend(q[r, h * D:(h + 1) * D], Kc[seq, hk, :n], Vc[seq, hk, :n], 0)
    return o, b


def step_ref(qkv, Kc, Vc, row_seq, row_pos, invf, Hq, Hk, mutant=None):
    """llm_attention_step.  qkv [R][(Hq + 2 Hk) 64] raw.  Returns o, bound [R][Hq 64], knew, kmag, vnew [R][Hk][64] (the cache
    rows the step appends, with the rotated key's error scale).  mutant: drop_cached (the last cached key) | drop_new | stale
    (the row at pos + 1 admitted) | seq0 | group | rot (the rotation taken at pos - 1)."""
    R = qkv.shape[0]
    o, b = np.full((R, Hq * D), np.nan), np.full((R, Hq * D), np.nan)
    knew, kmag, vnew = np.zeros((R, Hk, D)), np.zeros((R, Hk, D)), np.zeros((R, Hk, D))
    grp = Hq // Hk
    for r in range(R):
        seq, pos = (0 if mutant == "seq0" else row_seq[r]), row_pos[r]
        rp = pos - 1 if mutant == "rot" else pos
        if (mutant == "drop_cached" and pos < 1) or (mutant == "drop_new" and pos < 1) or (mutant == "stale" and pos + 1 >= Kc.shape[2]):
            continue
        for hk in range(Hk):
            knew[r, hk], kmag[r, hk] = rope(qkv[r, (Hq + hk) * D:(Hq + hk + 1) * D], rp, invf)
            vnew[r, hk] = qkv[r, (Hq + Hk + hk) * D:(Hq + Hk + hk + 1) * D]
        for h in range(Hq):
            hk = (h // grp + (1 if mutant == "group" else 0)) % Hk
            qr, _ = rope(qkv[r, h * D:(h + 1) * D], rp, invf)
            nc = pos - 1 if mutant == "drop_cached" else pos
            ks, vs = [Kc[seq, hk, :nc]], [Vc[seq, hk, :nc]]
            if mutant != "drop_new":
                ks.append(knew[r, hk][None]); vs.append(vnew[r, hk][None])
            if mutant == "stale":
                ks.append(Kc[seq, hk, pos + 1][None]); vs.append(Vc[seq, hk, pos + 1][None])
            o[r, h * D:(h + 1) * D], b[r, h * D:(h + 1) * D] = attend(qr, np.concatenate(ks), np.concatenate(vs), 16)
    return o, b, knew, kmag, vnew


PREFILL_POS = (0, 1, 62, 63, 64, 65, 127, 128, 129, 255, 256, 319)
STEP_POS = (0, 1, 2, 3, 4, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513)
HEADS = [(14, 2), (4, 2), (2, 2)]
PREFILL_CTX = 320
# (Hq, Hk, max_ctx, forms): the per-head (1) and the group (2) kernel forced; 0 = the launcher's rule, which at 14 / 2 heads and
# a context of 1100 has to take the per-head kernel (the group kernel's scores would need 77 KB of LDS)
STEP = [(14, 2, 640, (1, 2)), (4, 2, 640, (1, 2)), (2, 2, 640, (1, 2)), (16, 2, 520, (1, 2)), (14, 2, 1100, (0,))]


def _perm(n, tag):
    return np.argsort(synth.uniform("in.llmk.perm." + tag, (n,), 0.0, 1.0), kind="stable")


@functools.lru_cache(maxsize=None)
def _pool(name, shape):
    return synth.normal("in.llmk.attn." + name, shape).astype(np.float64)


@functools.lru_cache(maxsize=None)
def prefill_inputs(Hq, Hk):
    """about 20 rows over 3 sequences in permuted order: q [R][Hq 64], Kc, Vc [3][Hk][320][64], row_seq, row_pos (float64 / int)"""
    pos = np.array(list(PREFILL_POS) + [319, 0, 64, 129, 1, 255, 63, 128])
    R = len(pos)
    order = _perm(R, f"prefill.{Hq}")
    row_pos = pos[order]
    row_seq = (np.arange(R) * 7 + 1) % 3
    q = _pool("q", (24, 16 * D))[:R, :Hq * D]
    Kc, Vc = _pool("k", (24, 2, 1100, D))[:3, :Hk, :PREFILL_CTX], _pool("v", (24, 2, 1100, D))[:3, :Hk, :PREFILL_CTX]
    return q, Kc, Vc, row_seq.astype(np.int32), row_pos.astype(np.int32)


@functools.lru_cache(maxsize=None)
def step_inputs(Hq, Hk, max_ctx):
    """one row per position of STEP_POS and max_ctx - 1 (those below max_ctx), every row its own sequence, permuted"""
    pos = np.array([p for p in STEP_POS if p < max_ctx - 1] + [max_ctx - 1])
    R = len(pos)
    row_pos = pos[_perm(R, f"step.{Hq}.{max_ctx}")]
    row_seq = _perm(R, f"stepseq.{Hq}.{max_ctx}")
    qkv = _pool("qkv", (24, 20 * D))[:R, :(Hq + 2 * Hk) * D]
    Kc, Vc = _pool("k", (24, 2, 1100, D))[:R, :Hk, :max_ctx], _pool("v", (24, 2, 1100, D))[:R, :Hk, :max_ctx]
    return qkv, Kc, Vc, row_seq.astype(np.int32), row_pos.astype(np.int32)


# ---- fp32 emulations (the CPU test: the bounds are not tuned on a kernel) --------------------------------------------------------
def sum_f32(terms, order):
    """fp32 sum of terms [..., K] along the last axis: seq | rev | blocks (16-wide blocks, then the block sums) | perm"""
    t = np.asarray(terms, np.float32)
    K = t.shape[-1]
    if order == "rev":
        t = t[..., ::-1]
    if order == "perm":
        t = t[..., _perm(K, f"sum.{K}")]
    if order == "blocks":
        pad = (-K) % 16
        t = np.concatenate([t, np.zeros(t.shape[:-1] + (pad,), np.float32)], axis=-1).reshape(t.shape[:-1] + (-1, 16))
        return sum_f32(sum_f32(t, "seq"), "seq")
    acc = np.zeros(t.shape[:-1], np.float32)
    for k in range(t.shape[-1]):
        acc = (acc + t[..., k]).astype(np.float32)
    return acc


def attend_f32(q, keys, vals, order):
    """fp32 emulation of one (row, head): fp32 scores, exp, sums in `order`, one division"""
    q, keys, vals = (np.asarray(a, np.float32) for a in (q, keys, vals))
    s = (sum_f32(keys * q[None, :], order) * np.float32(SCALE)).astype(np.float32)
    p = np.exp((s - s.max()).astype(np.float32)).astype(np.float32)
    return (sum_f32((p[:, None] * vals).T, order) / sum_f32(p, order)).astype(np.float32)
