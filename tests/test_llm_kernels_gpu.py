"""The speech-token LM's decode products and cache attention, one operation at a time through the library's test hooks
(csrc/debug_llm.hip), against the float64 references of tests/llm_ref.py - reference, bounds with their derivation, inputs and
case lists are there; tests/test_llm_ref_cpu.py shows on the CPU that the exact cases are exact in every summation order, that
every plane of the split matters to every row and tile, and that the attention mutants leave the bound by a factor >= 4.

Every output, cache, image and workspace-free buffer is pre-filled with NaN or a sentinel and nothing outside the defined region
may change.  The shapes are chosen against the DEFAULT dispatch thresholds, so no FY_GV32_* variable and no FY_LLM_ATTN_GQA may
be set.  The worst |got - ref| / bound of each group goes to parity_llm_kernels.json (gpu_util.note); a ratio above 1 is a
finding about the kernel, not a reason to widen a bound.  The SwiGLU modes need an even N: at the odd shapes they run N - 1.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import llm_ref as lr
from fangyan_tts_amd import synth
from gpu_util import note

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SENT16 = 0x7B7B                            # bf16 1.3e36: finite, and no kernel output
FY_ERR_ARG = -1
NOTE = "parity_llm_kernels.json"


@pytest.fixture(autouse=True, scope="module")
def default_dispatch():
    bad = [k for k in os.environ if k.startswith("FY_GV32_") or k == "FY_LLM_ATTN_GQA"]
    assert not bad, f"{bad}: these tests are shaped against the default dispatch"


@functools.lru_cache(maxsize=1)
def hooks():
    from fangyan_tts_amd import _lib
    L = _lib.lib()
    vp, i32, f32 = C.c_void_p, C.c_int32, C.c_float
    L.fy_debug_gemv.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, f32, i32, vp, vp, i32, i32, vp, vp]
    L.fy_debug_gv32_split_rows.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp]
    L.fy_debug_gemv32.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp, i32, f32, vp, i32, vp, i32, vp, vp, vp, i32, vp, vp]
    L.fy_debug_llm_attention.argtypes = [vp, i32, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]
    L.fy_debug_llm_attention_step.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, i32, vp]
    for f in (L.fy_debug_gemv, L.fy_debug_gv32_split_rows, L.fy_debug_gemv32, L.fy_debug_llm_attention, L.fy_debug_llm_attention_step):
        f.restype = i32
    return L, _lib.check


def f32dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def u16dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint16).view(np.int16)).to(DEV)


def u16host(t):
    return t.cpu().numpy().view(np.uint16)


def ptr(t):
    return None if t is None else t.data_ptr()


def nan_f32(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def sent16(*shape):
    return torch.full(shape, SENT16, dtype=torch.int16, device=DEV)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def packed_scratch(N, K, planes=1):
    return torch.empty(planes * ((N + 31) // 32) * (K // 16) * 512, dtype=torch.int16, device=DEV)


def inputs(kind, N, K, pw=1, small=False):
    return lr.exact_inputs(N, K, 0, pw, small=small) if kind == "exact" else lr.random_inputs(N, K, pw)


def check_values(got, ref, exact_bits, tag, worst):
    assert np.isfinite(got).all(), tag
    if exact_bits:
        assert np.array_equal(ref.y.astype(np.float32).astype(np.float64), ref.y)
        assert same_bits(got, ref.y.astype(np.float32)), (tag, "not the float64 result bit for bit", float(np.abs(got - ref.y).max()))
    r = lr.ratio(got, ref.y, ref.bound)
    worst[0] = max(worst[0], r)
    assert r <= 1.0, (tag, r)


def check_planes(planes, ref, tag, worst):
    """planes [3][R][n] fp32: exactly split3 of an fp32 value inside the bound (llm_ref.SPLIT_EXACT_FROM: where a split can be exact)"""
    v64 = planes.astype(np.float64).sum(axis=0)
    v = v64.astype(np.float32)
    assert np.array_equal(v.astype(np.float64), v64), tag
    want = np.stack(lr.split3(v))
    bad = np.argwhere((want != planes).any(axis=0) & (np.abs(v) >= lr.SPLIT_EXACT_FROM))
    assert not len(bad), (tag, "not the exact split of one fp32 value", [(float(v[tuple(i)]), planes[(slice(None),) + tuple(i)].tolist(), want[(slice(None),) + tuple(i)].tolist()) for i in bad[:4]])
    check_values(v, ref, False, tag, worst)


# ---- 8-row products ------------------------------------------------------------------------------------------------------------
def run8(W, x, xsplit, R, N, K, bias, norm_w, mode, resid, pad, ws=0):
    """one gemv_bf16w call; returns y [R][n_out] (fp32) or the planes [3][R][n_out], and the counters (ws != 0)"""
    L, check = hooks()
    n_out = N // 2 if mode in (lr.GV_SWIGLU, lr.GV_SWIGLU_SPLIT) else N
    Z = (R + 7) // 8
    ldx = K + (8 if pad else 0)
    xd = xs = None
    if xsplit:
        xs = u16dev(lr.planes8_encode(x[:R].astype(np.float32), ldx))
    else:
        xh = np.full((R, ldx), np.nan, np.float32)
        xh[:, :K] = x[:R]
        xd = f32dev(xh)
    Wd, pk = f32dev(W), packed_scratch(N, K)
    bd, nd = (None if bias is None else f32dev(bias)), (None if norm_w is None else f32dev(norm_w))
    split_out = mode == lr.GV_SWIGLU_SPLIT
    ldy = n_out + ((8 if split_out else 3) if pad else 0)
    y = ysp = None
    if split_out:
        ysp = sent16(Z * 24 + 3, ldy)
    else:
        y = nan_f32(Z * 8 + 1, ldy)
        if mode == lr.GV_ADD:
            y[:R, :N] = f32dev(resid[:R])
    before = (ysp if split_out else y).clone()
    nct = Z * ((N + 31) // 32)
    cnt = torch.full((nct,), -1, dtype=torch.int32, device=DEV)
    check(L.fy_debug_gemv(ptr(Wd), ptr(pk), ptr(xd), ptr(xs), ldx, R, N, K, ptr(bd), ptr(nd), lr.EPS, mode, ptr(y), ptr(ysp), ldy, ws, ptr(cnt), None))
    torch.cuda.synchronize()
    if split_out:
        a, b = u16host(ysp), u16host(before)
        own = np.zeros(a.shape, bool)
        for p in range(3):
            for r in range(R):
                own[(r // 8) * 24 + p * 8 + r % 8, :n_out] = True
        assert np.array_equal(a[~own], b[~own]), "y_split written outside the rows and columns of the call"
        return lr.planes8_decode(a[:Z * 24], R, n_out), cnt.cpu().numpy()
    a, b = y.cpu().numpy(), before.cpu().numpy()
    own = np.zeros(a.shape, bool)
    own[:R, :n_out] = True
    assert same_bits(a[~own], b[~own]), "y written outside the rows and columns of the call"
    return a[:R, :n_out], cnt.cpu().numpy()


MODES8 = {lr.GV_STORE: "store", lr.GV_ADD: "add", lr.GV_SWIGLU: "swiglu", lr.GV_SWIGLU_SPLIT: "swiglu_split"}


@pytest.mark.parametrize("mode", list(MODES8), ids=list(MODES8.values()))
@pytest.mark.parametrize("N,K", lr.STAGED8)
def test_gemv8_staged(N, K, mode):
    sw = mode in (lr.GV_SWIGLU, lr.GV_SWIGLU_SPLIT)
    Nr = N - N % 2 if sw else N
    worst = [0.0]
    for kind in ("exact", "random") + (("exact-small",) if (N, K) == (896, 896) else ()):
        x, W, _, bias, resid, nw = inputs(kind.split("-")[0], N, K, small=kind.endswith("small"))
        for norm in (False, True):
            for with_bias in (False, True):
                ref = lr.product_ref(x[:20], W[:Nr], bias=bias[:Nr] if with_bias else None, resid=resid[:20, :Nr] if mode == lr.GV_ADD else None,
                                     norm_w=nw if norm else None, swiglu=sw, exact=kind != "random")
                for R in lr.R8:
                    tag = (kind, norm, with_bias, R)
                    got, _ = run8(W[:Nr], x, False, R, Nr, K, bias[:Nr] if with_bias else None, nw if norm else None, mode, resid[:, :Nr], pad=R == 9)
                    refR = lr.Prod(ref.y[:R], ref.bound[:R], None, None, None)
                    if mode == lr.GV_SWIGLU_SPLIT:
                        check_planes(got, refR, tag, worst)
                    else:
                        check_values(got, refR, kind != "random" and not norm and not sw, tag, worst)
    note(NOTE, f"gemv8.staged.{N}x{K}.{MODES8[mode]}", worst[0])


@pytest.mark.parametrize("N,K,ws", lr.DIRECT8)
def test_gemv8_presplit_split_k(N, K, ws):
    worst = [0.0]
    for kind in ("exact", "random"):
        x, W, _, bias, resid, _ = inputs(kind, N, K)
        for mode in (lr.GV_STORE, lr.GV_ADD, lr.GV_SWIGLU, lr.GV_SWIGLU_SPLIT):
            sw = mode in (lr.GV_SWIGLU, lr.GV_SWIGLU_SPLIT)
            ref = lr.product_ref(x[:20], W, bias=bias, resid=resid[:20] if mode == lr.GV_ADD else None, swiglu=sw, exact=kind == "exact")
            for R in lr.R8:
                tag = (kind, mode, R)
                refR = lr.Prod(ref.y[:R], ref.bound[:R], None, None, None)
                got, cnt = run8(W, x, True, R, N, K, bias, None, mode, resid, pad=R == 9, ws=1 if ws else 0)
                if mode == lr.GV_SWIGLU_SPLIT:
                    check_planes(got, refR, tag, worst)
                else:
                    check_values(got, refR, kind == "exact" and not sw, tag, worst)
                if ws:
                    assert not cnt.any(), (tag, "arrival counters not re-armed", cnt)
                    again, cnt = run8(W, x, True, R, N, K, bias, None, mode, resid, pad=R == 9, ws=2)      # the same workspace, as the first call left it
                    assert same_bits(again, got), (tag, "second call on the same workspace differs")
                    assert not cnt.any(), (tag, "arrival counters not re-armed by the second call", cnt)
    note(NOTE, f"gemv8.presplit.{N}x{K}", worst[0])


# ---- 32-row products -----------------------------------------------------------------------------------------------------------
def run32(W, W_lo, img, R, N, K, mode, bias=None, resid=None, ssq=None, ln_next=None, want_img=False, ws=0, pad=False):
    """one gemv32 call on a caller-built operand image.  Returns y [R][N] (or None), the output image (uint16, or None), ssq_out, counters."""
    L, check = hooks()
    Z, T = (R + 31) // 32, (N + 31) // 32
    pk = packed_scratch(N, K, 2 if W_lo is not None else 1)
    Wd, Wl = f32dev(W), (None if W_lo is None else f32dev(W_lo))
    imgd = u16dev(img)
    ldy = N + (4 if pad else 0)
    y = before = None
    if mode != lr.GV32_SWIGLU_IMG:
        y = nan_f32(R + 1, ldy)
        if mode == lr.GV32_ADD_IMG:
            y[:R, :N] = f32dev(resid[:R])
        before = y.clone()
    n_img = N // 2 if mode == lr.GV32_SWIGLU_IMG else N
    io = so = None
    if want_img or mode == lr.GV32_SWIGLU_IMG:
        io = sent16(Z * (n_img // 16) * 3 * 512 + 8)
        if mode == lr.GV32_ADD_IMG:
            so = nan_f32(T * 32 * Z + 1)
    ssqd = None if ssq is None else f32dev(ssq)
    bd, ld = (None if bias is None else f32dev(bias)), (None if ln_next is None else f32dev(ln_next))
    cnt = torch.full((Z * T,), -1, dtype=torch.int32, device=DEV)
    check(L.fy_debug_gemv32(ptr(Wd), ptr(Wl), ptr(pk), ptr(imgd), R, N, K, ptr(ssqd), 0 if ssq is None else ssq.shape[0], lr.EPS, ptr(bd),
                            mode, ptr(y), ldy, ptr(ld), ptr(io), ptr(so), ws, ptr(cnt), None))
    torch.cuda.synchronize()
    yh = None
    if y is not None:
        a, b = y.cpu().numpy(), before.cpu().numpy()
        own = np.zeros(a.shape, bool)
        own[:R, :N] = True
        assert same_bits(a[~own], b[~own]), "y written outside the rows and columns of the call"
        yh = a[:R, :N]
    ih = sh = None
    if io is not None:
        ih = u16host(io)
        assert (ih[-8:] == SENT16).all(), "image written past its end"
        ih = ih[:-8]
    if so is not None:
        sh = so.cpu().numpy()
        assert np.isnan(sh[-1]), "ssq_out written past its end"
        sh = sh[:-1].reshape(T, 32 * Z)
    return yh, ih, sh, cnt.cpu().numpy()


def twice32(ws, tag, *args, **kw):
    out = run32(*args, ws=1 if ws else 0, **kw)
    if ws:
        assert not out[3].any(), (tag, "arrival counters not re-armed", out[3])
        again = run32(*args, ws=2, **kw)
        assert not again[3].any(), (tag, "arrival counters not re-armed by the second call")
        for a, b in zip(out[:3], again[:3]):
            assert (a is None and b is None) or np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b), \
                (tag, "second call on the same workspace differs")
    return out


def check_image_padding(pl, R, tag):
    assert not pl[:, R:].any(), (tag, "image rows beyond R are not zero")


CASES32 = [(n, N, K, ws, 1) for n, N, K, ws in lr.FORMS32] + [(n + "-xw", N, K, False, 2) for n, N, K in lr.XW32]


@pytest.mark.parametrize("name,N,K,ws,pw", CASES32, ids=[c[0] for c in CASES32])
def test_gemv32_forms(name, N, K, ws, pw):
    worst = {"store": [0.0], "add_img": [0.0], "swiglu_img": [0.0], "ssq_out": 0.0}
    for kind in ("exact", "random"):
        x, W, W_lo, bias, resid, nw = inputs(kind, N, K, pw)
        exact = kind == "exact"
        ln_next = synth.normal("in.llmk.ln_next", (N,), 1.0, 0.25)
        refs = {"store": lr.product_ref(x, W, W_lo, bias=bias, exact=exact)}
        if N % 32 == 0:
            refs["add_img"] = lr.product_ref(x, W, W_lo, resid=resid, exact=exact)
            refs["swiglu_img"] = lr.product_ref(x, W, W_lo, swiglu=True, exact=exact)
        for R in lr.R32:
            img = lr.image_of(x[:R].astype(np.float32))
            for m, ref in refs.items():
                tag = (kind, m, R)
                refR = lr.Prod(ref.y[:R], ref.bound[:R], None, None, None)
                if m == "store":
                    y, _, _, _ = twice32(ws, tag, W, W_lo, img, R, N, K, lr.GV32_STORE, bias=bias, pad=R == 9)
                    check_values(y, refR, exact, tag, worst[m])
                elif m == "add_img":
                    y, io, so, _ = twice32(ws, tag, W, W_lo, img, R, N, K, lr.GV32_ADD_IMG, resid=resid, ln_next=ln_next, want_img=True, pad=R == 9)
                    check_values(y, refR, exact, tag, worst[m])
                    pl = lr.image_decode(io, R, N)
                    want = (y * ln_next.astype(np.float32)[None, :]).astype(np.float32)
                    assert np.array_equal(pl[:, :R], np.stack(lr.split3(want))), (tag, "img_out is not split3(ln_next * y_new)")
                    check_image_padding(pl, R, tag)
                    sref = lr.ssq_ref(y.astype(np.float64))
                    rel = float((np.abs(so[:, :R] - sref) / (lr.SSQ_REL * sref + 1e-30)).max())
                    worst["ssq_out"] = max(worst["ssq_out"], rel)
                    assert rel <= 1.0, (tag, "ssq_out", rel)
                    assert not so[:, R:].any(), (tag, "ssq_out rows beyond R are not zero")
                    y2, io2, so2, _ = run32(W, W_lo, img, R, N, K, lr.GV32_ADD_IMG, resid=resid, ws=1 if ws else 0)       # without img_out: the same sums
                    assert same_bits(y2, y) and io2 is None
                else:
                    _, io, _, _ = twice32(ws, tag, W, W_lo, img, R, N, K, lr.GV32_SWIGLU_IMG)
                    pl = lr.image_decode(io, R, N // 2)
                    check_planes(pl[:, :R], refR, tag, worst[m])
                    check_image_padding(pl, R, tag)
    for m, w in worst.items():
        note(NOTE, f"gemv32.{name}.{m}", w if isinstance(w, float) else w[0])


@pytest.mark.parametrize("N,K", [(896, 896), (64, 1024)])
def test_gemv32_store_fused_norm(N, K):
    """GV32_STORE on the image of norm_w x with K / 32 partial sums of squares per row: 28, and 32 - the most the kernel takes"""
    worst = [0.0]
    for kind in ("exact", "exact-small", "random"):
        if kind == "exact-small" and K != 896:
            continue
        x, W, _, bias, _, nw = inputs(kind.split("-")[0], N, K, small=kind.endswith("small"))
        for fused in (True, False):
            ref = lr.product_ref(x, W, bias=bias, norm_w=nw if fused else None, exact=kind != "random")
            for R in lr.R32:
                Z = (R + 31) // 32
                xn = (x[:R].astype(np.float32) * nw.astype(np.float32)).astype(np.float32) if fused else x[:R].astype(np.float32)
                ssq = None
                if fused:
                    ssq = np.zeros((K // 32, 32 * Z), np.float32)
                    ssq[:, :R] = lr.ssq_ref(x[:R])
                y, _, _, _ = run32(W, None, lr.image_of(xn), R, N, K, lr.GV32_STORE, bias=bias, ssq=ssq)
                check_values(y, lr.Prod(ref.y[:R], ref.bound[:R], None, None, None), kind != "random" and not fused, (kind, fused, R), worst)
    note(NOTE, f"gemv32.fused_norm.{N}x{K}", worst[0])


@pytest.mark.parametrize("K", [128, 896])
def test_gv32_split_rows_image_and_ssq(K):
    L, check = hooks()
    worst = 0.0
    for kind in ("exact", "random"):
        x, _, _, _, _, nw = inputs(kind, 64, K) if K == 128 else inputs(kind, 896, K)
        for with_ln in (False, True):
            for with_ssq in (False, True):
                for R in lr.R32:
                    Z, ldx = (R + 31) // 32, K + (4 if R == 9 else 0)
                    xh = np.full((R, ldx), np.nan, np.float32)
                    xh[:, :K] = x[:R]
                    n_el = Z * (K // 16) * 3 * 512
                    img, ssq = sent16(n_el + 8), nan_f32((K // 32) * 32 * Z + 1)
                    xd, nd = f32dev(xh), f32dev(nw)
                    check(L.fy_debug_gv32_split_rows(ptr(xd), ldx, R, K, ptr(nd) if with_ln else None, ptr(img), ptr(ssq) if with_ssq else None, None))
                    torch.cuda.synchronize()
                    ih = u16host(img)
                    assert (ih[-8:] == SENT16).all()
                    want = (x[:R].astype(np.float32) * nw.astype(np.float32)).astype(np.float32) if with_ln else x[:R].astype(np.float32)
                    pl = lr.image_decode(ih[:-8], R, K)                    # compared as values: a padding row of -0 is zero
                    assert np.array_equal(pl[:, :R], np.stack(lr.split3(want))) and not pl[:, R:].any(), (kind, with_ln, R, "the image is not the exact split in gemv32.h's layout")
                    sh = ssq.cpu().numpy()
                    if not with_ssq:
                        assert np.isnan(sh).all()
                        continue
                    assert np.isnan(sh[-1])
                    sh = sh[:-1].reshape(K // 32, 32 * Z)
                    sref = lr.ssq_ref(x[:R])
                    rel = float((np.abs(sh[:, :R] - sref) / (lr.SSQ_REL * sref + 1e-30)).max())
                    worst = max(worst, rel)
                    assert rel <= 1.0 and not sh[:, R:].any(), (kind, with_ln, R, rel)
    note(NOTE, f"gv32_split_rows.{K}.ssq", worst)


# ---- cache attention -----------------------------------------------------------------------------------------------------------
def poisoned_cache(Kc, Vc, row_seq, row_pos, keep_pos):
    """float32 copies with NaN in every row past the largest position a sequence is read at (keep_pos: that row itself stays)"""
    Kp, Vp = Kc.astype(np.float32).copy(), Vc.astype(np.float32).copy()
    last = np.full(Kc.shape[0], -1)
    for s, p in zip(row_seq, row_pos):
        last[s] = max(last[s], p)
    for s in range(Kc.shape[0]):
        first = last[s] + (1 if keep_pos else 0)
        Kp[s, :, first:], Vp[s, :, first:] = np.nan, np.nan
    return Kp, Vp


@pytest.mark.parametrize("Hq,Hk", lr.HEADS)
def test_prefill_attention(Hq, Hk):
    L, check = hooks()
    q, Kc, Vc, row_seq, row_pos = lr.prefill_inputs(Hq, Hk)
    o, bound = lr.attention_ref(q, Kc, Vc, row_seq, row_pos, Hq, Hk)
    R, pad = len(row_pos), (8 if Hq == 4 else 0)
    Kp, Vp = poisoned_cache(Kc, Vc, row_seq, row_pos, True)
    qh = np.full((R, Hq * 64 + pad), np.nan, np.float32)
    qh[:, :Hq * 64] = q
    out = nan_f32(R + 1, Hq * 64 + pad)
    Kd, Vd, qd = f32dev(Kp), f32dev(Vp), f32dev(qh)
    sd, pd = torch.from_numpy(row_seq).to(DEV), torch.from_numpy(row_pos).to(DEV)
    check(L.fy_debug_llm_attention(ptr(qd), Hq * 64 + pad, ptr(Kd), ptr(Vd), ptr(sd), ptr(pd),
                                   ptr(out), Hq * 64 + pad, R, Hq, Hk, lr.PREFILL_CTX, None))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.isnan(got[R]).all() and np.isnan(got[:, Hq * 64:]).all()
    assert same_bits(Kd.cpu().numpy(), Kp) and same_bits(Vd.cpu().numpy(), Vp)
    got = got[:R, :Hq * 64]
    assert np.isfinite(got).all()
    r = lr.ratio(got, o, bound)
    note(NOTE, f"attention.prefill.{Hq}_{Hk}", r)
    assert r <= 1.0, r


STEP_CASES = [(Hq, Hk, ctx, f) for Hq, Hk, ctx, forms in lr.STEP for f in forms]


@pytest.mark.parametrize("Hq,Hk,ctx,form", STEP_CASES, ids=[f"{a}_{b}-ctx{c}-form{f}" for a, b, c, f in STEP_CASES])
def test_step_attention(Hq, Hk, ctx, form):
    L, check = hooks()
    qkv, Kc, Vc, row_seq, row_pos = lr.step_inputs(Hq, Hk, ctx)
    invf = lr.inv_freq()
    o, bound, knew, kmag, vnew = lr.step_ref(qkv, Kc, Vc, row_seq, row_pos, invf, Hq, Hk)
    R = len(row_pos)
    Kp, Vp = poisoned_cache(Kc, Vc, row_seq, row_pos, False)
    qd, fd = f32dev(qkv), f32dev(invf)
    sd, pd = torch.from_numpy(row_seq).to(DEV), torch.from_numpy(row_pos).to(DEV)
    results = {}
    for path in ("out", "img"):
        Kd, Vd = f32dev(Kp), f32dev(Vp)
        out = nan_f32(R + 1, Hq * 64 + 4) if path == "out" else None
        img = sent16(((R + 31) // 32) * Hq * 4 * 3 * 512 + 8) if path == "img" else None
        check(L.fy_debug_llm_attention_step(ptr(qd), ptr(Kd), ptr(Vd), ptr(sd), ptr(pd), ptr(fd), ptr(out), Hq * 64 + 4, R, Hq, Hk, ctx, ptr(img), form, None))
        torch.cuda.synchronize()
        Kg, Vg = Kd.cpu().numpy(), Vd.cpu().numpy()
        own = np.zeros(Kg.shape, bool)
        for r in range(R):
            s, p = row_seq[r], row_pos[r]
            own[s, :, p] = True
            assert (np.abs(Kg[s, :, p] - knew[r]) <= 8 * lr.U * kmag[r] + 1e-30).all(), (path, r, "the appended key is not the rotated k within 4 ulp")
            assert same_bits(Vg[s, :, p], vnew[r].astype(np.float32)), (path, r, "the appended value is not v")
        assert same_bits(Kg[~own], Kp[~own]) and same_bits(Vg[~own], Vp[~own]), (path, "the cache changed outside the appended rows")
        results[path + ".K"] = Kg
        if path == "out":
            got = out.cpu().numpy()
            assert np.isnan(got[R]).all() and np.isnan(got[:, Hq * 64:]).all()
            results["out"] = got[:R, :Hq * 64]
        else:
            ih = u16host(img)
            assert (ih[-8:] == SENT16).all()
            results["img"] = ih[:-8]
    got = results["out"]
    assert np.isfinite(got).all()
    r = lr.ratio(got, o, bound)
    note(NOTE, f"attention.step.{Hq}_{Hk}.ctx{ctx}.form{form}", r)
    assert r <= 1.0, r
    assert same_bits(results["img.K"], results["out.K"])
    # the image path writes the pieces of its own rows only: rows beyond R keep the sentinel
    pl_bits = np.asarray(results["img"]).reshape((R + 31) // 32, Hq * 4, 3, 2, 32, 8).transpose(2, 0, 4, 1, 3, 5).reshape(3, -1, Hq * 64)
    assert np.array_equal(pl_bits[:, :R], lr.bits(np.stack(lr.split3(got)))), "the image is not split3 of the out path's result"
    assert (pl_bits[:, R:] == SENT16).all()


def test_step_attention_group_form_refuses_what_does_not_fit():
    L, _ = hooks()
    z = torch.zeros(16 * 64 * 2, device=DEV)
    i = torch.zeros(2, dtype=torch.int32, device=DEV)
    assert L.fy_debug_llm_attention_step(ptr(z), ptr(z), ptr(z), ptr(i), ptr(i), ptr(z), ptr(z), 14 * 64, 1, 14, 2, 1100, None, 2, None) == FY_ERR_ARG
    assert L.fy_debug_llm_attention_step(ptr(z), ptr(z), ptr(z), ptr(i), ptr(i), ptr(z), ptr(z), 14 * 64, 1, 14, 2, 640, None, 3, None) == FY_ERR_ARG
