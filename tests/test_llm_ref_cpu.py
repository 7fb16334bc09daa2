"""The direct LM kernel tests (tests/test_llm_kernels_gpu.py) can fail, and their bounds are not tuned on the kernels:

* every exact product case keeps max |x| |W|^T under its limit (the builder asserts it, for every row and column), NumPy fp32
  sums in four orders reproduce float64 bit for bit (every row; the first 64 and the last 33 columns, the ragged tile among
  them - the limit above is what makes it hold everywhere), and dropping ANY plane of x - or the second weight plane - changes an output in every row
  and every 32-column tile;
* the layouts round-trip and the planes add up to x;
* an fp32 NumPy emulation of the random cases stays within 1.0 of the product bound and of the attention bound;
* for every attention case each mutant - a cached key dropped, the new key dropped, one stale key admitted, row_seq ignored,
  the kv group off by one, the rotation at pos - 1 - leaves the bound by a factor >= 4 (a condition on the chosen inputs: a
  case that cannot reach it is changed, not the factor).
"""
import numpy as np
import pytest

import llm_ref as lr

FACTOR = 4.0
ORDERS = ("seq", "rev", "blocks", "perm")
ROWS = 9                                            # rows of the builders' 40 that the emulations of the random cases walk

EXACT = sorted({(N, K, 1) for N, K in lr.STAGED8} | {(N, K, 1) for N, K, _ in lr.DIRECT8} | {(N, K, 1) for _, N, K, _ in lr.FORMS32}
               | {(N, K, 2) for _, N, K in lr.XW32})


def _tiles_changed(y0, y1):
    """bool [rows][tiles]: some output of the row differs inside the 32-column tile"""
    R, N = y0.shape
    pad = (-N) % 32
    d = np.pad(y0 != y1, ((0, 0), (0, pad))).reshape(R, -1, 32)
    return d.any(axis=2)


@pytest.mark.parametrize("N,K,pw", EXACT)
def test_exact_cases_are_exact_in_every_order_and_every_plane_matters(N, K, pw):
    x, W, W_lo, bias, resid, _ = lr.exact_inputs(N, K, 0, pw)
    cols = np.r_[0:min(N, 64), N - min(N, 33):N]                             # the summation orders: a slice of the columns is enough
    Wt = W if W_lo is None else W + W_lo
    ref = x @ Wt[cols].T
    terms = (x[:, None, :] * Wt[None, cols, :])
    assert np.array_equal(terms.astype(np.float32).astype(np.float64), terms)
    for order in ORDERS:
        got = lr.sum_f32(terms, order)
        assert np.array_equal(got.astype(np.float64), ref), order
    y = (ref + bias[cols]).astype(np.float32)
    assert np.array_equal(y.astype(np.float64), ref + bias[cols])
    y = (resid[:, cols] + ref).astype(np.float32)
    assert np.array_equal(y.astype(np.float64), resid[:, cols] + ref)
    planes = np.stack(lr.split3(x.astype(np.float32))).astype(np.float64)
    assert np.array_equal(planes.sum(axis=0), x)
    full = x @ Wt.T
    for p in range(3 if pw == 1 else 2):
        dropped = (planes.sum(axis=0) - planes[p]) @ Wt.T
        assert _tiles_changed(full, dropped).all(), f"x plane {p}"
    if pw == 2:
        assert _tiles_changed(full, x @ W.T).all(), "second weight plane"


def test_small_rows_keep_the_inputs_exact_and_make_eps_matter():
    x, W, _, _, _, nw = lr.exact_inputs(896, 896, 0, 1, small=True)
    x0 = lr.exact_inputs(896, 896, 0, 1)[0]
    assert np.array_equal(x * 2.0 ** 10, x0)
    with_eps = lr.product_ref(x, W, norm_w=nw, exact=True)
    without = lr.product_ref(x, W, norm_w=nw, eps=0.0, exact=True)
    assert lr.ratio(without.y, with_eps.y, with_eps.bound) >= FACTOR


def test_layouts_round_trip():
    x = lr.random_inputs(64, 128)[0].astype(np.float32)
    for R in (1, 31, 32, 33, 40):
        img = lr.image_of(x[:R])
        assert img.shape == ((R + 31) // 32, 8, 3, 64, 8)
        pl = lr.image_decode(img, R, 128)
        assert np.array_equal(pl.astype(np.float64).sum(axis=0)[:R], x[:R].astype(np.float64))
        assert not pl[:, R:].any()
        # lane l of fragment kk: row l & 31, columns 16 kk + 8 (l >> 5) ..
        kk, l, j = 5, 37, 3
        assert img[0, kk, 1, l, j] == lr.bits(lr.split3(x[l & 31] if (l & 31) < R else np.zeros(128, np.float32))[1])[16 * kk + 8 * (l >> 5) + j]
    for R in (1, 8, 9, 20):
        buf = lr.planes8_encode(x[:R], 136)
        assert buf.shape == ((R + 7) // 8, 24, 136)
        assert np.array_equal(lr.planes8_decode(buf, R, 128).astype(np.float64).sum(axis=0), x[:R].astype(np.float64))


@pytest.mark.parametrize("N,K,pw", [(64, 128, 1), (101, 1024, 1), (64, 2064, 1), (64, 2128, 2)])
def test_fp32_emulation_stays_inside_the_product_bound(N, K, pw):
    x, W, W_lo, bias, resid, nw = lr.random_inputs(N, K, pw)
    x = x[:ROWS]
    Wt = W if W_lo is None else W + W_lo
    for norm in (False, True):
        ref = lr.product_ref(x, W, W_lo, bias=bias, resid=resid[:ROWS], norm_w=nw if norm else None)
        xn = (x.astype(np.float32) * nw.astype(np.float32)) if norm else x.astype(np.float32)
        terms = xn[:, None, :].astype(np.float64) * Wt[None]                       # exact products, as the split gives them
        for order in ("seq", "blocks"):
            acc = lr.sum_f32(terms, order)
            if norm:
                ss = lr.sum_f32((x.astype(np.float32) ** 2).astype(np.float32), order)
                acc = acc * (np.float32(1) / np.sqrt(ss / np.float32(K) + np.float32(lr.EPS), dtype=np.float32))[:, None]
            got = resid[:ROWS].astype(np.float32) + (acc + bias.astype(np.float32))
            assert lr.ratio(got, ref.y, ref.bound) <= 1.0, (norm, order)


def test_swiglu_emulation_stays_inside_the_bound():
    x, W, _, bias, _, _ = lr.exact_inputs(64, 128)
    ref = lr.product_ref(x, W, bias=bias, swiglu=True, exact=True)
    g, u = ref.g.astype(np.float32), ref.u.astype(np.float32)
    got = (g / (np.float32(1) + np.exp(-g, dtype=np.float32))).astype(np.float32) * u
    assert lr.ratio(got, ref.y, ref.bound) <= 1.0
    assert lr.ratio(ref.g * ref.u * 0.5, ref.y, ref.bound) >= FACTOR             # a wrong activation leaves it


def _worst(om, o, b):
    ok = np.isfinite(om)
    return float((np.abs(om - o)[ok] / b[ok]).max()) if ok.any() else 0.0


@pytest.mark.parametrize("Hq,Hk", lr.HEADS)
def test_prefill_attention_mutants_and_emulation(Hq, Hk):
    q, Kc, Vc, row_seq, row_pos = lr.prefill_inputs(Hq, Hk)
    o, b = lr.attention_ref(q, Kc, Vc, row_seq, row_pos, Hq, Hk)
    assert np.isfinite(o).all()
    for m in ("drop_last", "stale", "seq0") + ("group",):
        om, _ = lr.attention_ref(q, Kc, Vc, row_seq, row_pos, Hq, Hk, mutant=m)
        assert _worst(om, o, b) >= FACTOR, m
    worst = 0.0
    for r in range(0, len(row_pos), 3):
        for h in (0, Hq - 1):
            hk, n = h // (Hq // Hk), row_pos[r] + 1
            for order in ("seq", "blocks"):
                got = lr.attend_f32(q[r, h * 64:(h + 1) * 64], Kc[row_seq[r], hk, :n], Vc[row_seq[r], hk, :n], order)
                worst = max(worst, float((np.abs(got - o[r, h * 64:(h + 1) * 64]) / b[r, h * 64:(h + 1) * 64]).max()))
    assert worst <= 1.0, worst


@pytest.mark.parametrize("Hq,Hk,ctx,forms", lr.STEP, ids=lambda v: str(v))
def test_step_attention_mutants_and_emulation(Hq, Hk, ctx, forms):
    qkv, Kc, Vc, row_seq, row_pos = lr.step_inputs(Hq, Hk, ctx)
    invf = lr.inv_freq()
    o, b, knew, kmag, vnew = lr.step_ref(qkv, Kc, Vc, row_seq, row_pos, invf, Hq, Hk)
    assert np.isfinite(o).all() and sorted(row_seq) == list(range(len(row_pos)))
    for m in ("drop_cached", "drop_new", "stale", "seq0", "group", "rot"):
        om = lr.step_ref(qkv, Kc, Vc, row_seq, row_pos, invf, Hq, Hk, mutant=m)[0]
        assert _worst(om, o, b) >= FACTOR, m
    worst = 0.0
    for r in range(0, len(row_pos), 4):
        pos, h = row_pos[r], Hq - 1
        hk = h // (Hq // Hk)
        # fp32 rotation: float32 sin / cos of the fp32 angle, products and sums in fp32
        ang = (np.float32(pos) * invf).astype(np.float32)
        c, s = np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)

        def rot(x):
            x = x.astype(np.float32)
            return np.concatenate([x[:32] * c - x[32:] * s, x[32:] * c + x[:32] * s]).astype(np.float32)
        qr, kr = rot(qkv[r, h * 64:(h + 1) * 64]), rot(qkv[r, (Hq + hk) * 64:(Hq + hk + 1) * 64])
        assert (np.abs(kr - knew[r, hk]) <= 8 * lr.U * kmag[r, hk] + 1e-30).all()
        keys = np.concatenate([Kc[row_seq[r], hk, :pos], kr[None].astype(np.float64)])
        vals = np.concatenate([Vc[row_seq[r], hk, :pos], vnew[r, hk][None]])
        for order in ("seq", "blocks"):
            got = lr.attend_f32(qr, keys, vals, order)
            worst = max(worst, float((np.abs(got - o[r, h * 64:(h + 1) * 64]) / b[r, h * 64:(h + 1) * 64]).max()))
    assert worst <= 1.0, worst
