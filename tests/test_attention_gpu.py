"""The DiT attention kernels, called directly through the library's test hooks, against the float64 reference of
tests/attn_ref.py (reference, bounds, inputs and case lists; tests/test_attention_ref_cpu.py shows that a mask off by one key
leaves these bounds by a factor >= 4 on every case here).

Every call is poisoned: the qkv rows at or past a sequence's length are NaN (the kernels clamp their reads to len - 1 and must
not consume them), and the output is pre-filled with a sentinel bit pattern that every row the call does not own must keep.

Per-element bounds: 2^-8 (|o| + a) + 1e-6 for the bf16 kernels, 2^-14 (|o| + a) for the split ones.  Every case records its
largest |got - o| / bound in parity_attn.json (gpu_util.note).  The NumPy emulation of the bf16 kernels' rounding
(attn_ref.emulate) gives 0.20 (flat, 650 frames) to 0.85 (falling, 7-frame chunks) of the bf16 bound over these cases, and a
float64 attention rounded once to hi + lo gives 0.06 of the split bound; a ratio above 1 is a finding about the kernel, not a
reason to widen a bound.
"""
import ctypes as C
import functools

import pytest
import torch

import attn_ref as ar
from gpu_util import note

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SENTINEL = 0x7B7B                          # bf16 1.3e36: finite, and no kernel output


@functools.lru_cache(maxsize=1)
def hooks():
    from fangyan_tts_amd import _lib
    L = _lib.lib()
    vp, i32 = C.c_void_p, C.c_int32
    L.fy_debug_dit_attention.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp]
    L.fy_debug_dit_attention_tab.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]
    L.fy_debug_dit_attention_split.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]
    L.fy_debug_dit_attention_split_tab.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]
    for f in (L.fy_debug_dit_attention, L.fy_debug_dit_attention_tab, L.fy_debug_dit_attention_split, L.fy_debug_dit_attention_split_tab):
        f.restype = i32
    return L, _lib.check


@functools.lru_cache(maxsize=4)
def _reference(lens, chunk, mode, H):
    """(X, [(o, a)] per sequence): computed once per (lengths, chunk, inputs), shared by the forms and the tests."""
    if mode == "split":
        hi, lo = ar.inputs_split(list(lens), H)
        return (hi, lo), ar.ref_batch(hi.double() + lo.double(), lens, chunk)
    X = ar.inputs(list(lens), mode, H)
    return X, ar.ref_batch(X, lens, chunk)


def reference(lens, chunk, mode="default", H=2):
    return _reference(tuple(lens), chunk, mode, H)


def sentinel(rows, cols):
    return torch.full((rows, cols), SENTINEL, dtype=torch.int16, device=DEV).view(torch.bfloat16)


def bits(x):
    return x.view(torch.int16).cpu()


def pack(X, lens, interleaved=False):
    """[nseq][Tmax][3][H][64] -> device bf16 rows [q | k | v]; row t of sequence s at s Tmax + t, or at nseq t + s; NaN past len."""
    X = X.clone()
    for s, n in enumerate(lens):
        X[s, n:] = float("nan")
    if interleaved:
        X = X.transpose(0, 1)
    return X.reshape(X.shape[0] * X.shape[1], -1).to(torch.bfloat16).to(DEV).contiguous()


def unpack(out, nseq, interleaved=False):
    """device [rows][H * 64] -> cpu int16 bits [nseq][Tmax][H][64]"""
    b = bits(out)
    b = b.view(-1, nseq, b.shape[1] // ar.D, ar.D).transpose(0, 1) if interleaved else b.view(nseq, -1, b.shape[1] // ar.D, ar.D)
    return b.contiguous()


def as_float(b):
    return b.view(torch.bfloat16).float()


def run_direct(qkv, lens_dev, nseq, Tmax, H, chunk, q_begin, interleaved, kernel, waves):
    L, check = hooks()
    out = sentinel(nseq * Tmax, H * ar.D)
    check(L.fy_debug_dit_attention(qkv.data_ptr(), out.data_ptr(), lens_dev.data_ptr(), nseq, Tmax, H, chunk, q_begin, int(interleaved), kernel, waves, None))
    torch.cuda.synchronize()
    return unpack(out, nseq, interleaved)


def check_rows(got_bits, lens, refs, bound, q_begin=0):
    """Owned rows (q_begin <= t < len) finite and inside the bound; every other row still the sentinel.  The largest ratio."""
    worst = 0.0
    for s, n in enumerate(lens):
        lo = min(q_begin, n)
        assert (got_bits[s, :lo] == SENTINEL_I16).all() and (got_bits[s, n:] == SENTINEL_I16).all(), f"sequence {s}: a row outside [{lo}, {n}) was written"
        if lo < n:
            got = as_float(got_bits[s, lo:n])
            assert torch.isfinite(got).all(), f"sequence {s}: non-finite output"
            o, a = refs[s]
            worst = max(worst, ar.ratio(got, o[lo:], bound(o[lo:], a[lo:])))
    return worst


SENTINEL_I16 = torch.tensor(SENTINEL, dtype=torch.int16)


def forms(Tmax):
    """(kernel, waves): round 5 at four waves, at eight, automatic; round 2 at four waves and as one workgroup per (sequence, head)"""
    nw = -(-Tmax // 32)
    return [(0, 4), (0, 8), (0, 0), (1, 4)] + ([(1, nw)] if 8 <= nw <= 16 else [])


@pytest.mark.parametrize("c", ar.DIRECT, ids=ar.cid)
def test_dit_attention_against_float64(c):
    """Both kernels in every workgroup form on ragged batches: inside the bound, nothing written outside the sequences, and the
    forms of one kernel bit-identical (attn_dit.hip: a query's result does not depend on the launch grid)."""
    nseq, Tmax = len(c.lens), max(c.lens)
    X, refs = reference(c.lens, c.chunk, c.mode, c.H)
    qkv = pack(X, c.lens)
    lens_dev = torch.tensor(c.lens, dtype=torch.int32, device=DEV)
    outs, ratios = {}, {}
    for kernel, waves in forms(Tmax):
        outs[kernel, waves] = run_direct(qkv, lens_dev, nseq, Tmax, c.H, c.chunk, 0, False, kernel, waves)
        ratios[f"k{kernel}w{waves}"] = check_rows(outs[kernel, waves], c.lens, refs, ar.bound_bf16)
    print(ar.cid(c), ratios)
    note("parity_attn.json", f"direct.{ar.cid(c)}", max(ratios.values()))
    assert max(ratios.values()) <= 1.0, ratios
    for (kernel, waves), out in outs.items():
        assert torch.equal(out, outs[kernel, 4]), f"kernel {kernel}: the {waves}-wave form differs from the four-wave form"


@pytest.mark.parametrize("lens,chunk,interleaved", ar.QBEGIN, ids=lambda v: str(v).replace(" ", ""))
def test_dit_attention_q_begin(lens, chunk, interleaved):
    """Incremental calls (q_begin > 0; interleaved with two sequences is the flow decoder's own): only the rows from q_begin on are
    written, inside the bound and bit-identical to the same rows of the q_begin = 0 call of the same kernel and form."""
    nseq, Tmax, H = len(lens), max(lens), 2
    X, refs = reference(lens, chunk)
    qkv = pack(X, lens, interleaved)
    lens_dev = torch.tensor(lens, dtype=torch.int32, device=DEV)
    worst = 0.0
    for kernel, waves in forms(Tmax):
        full = run_direct(qkv, lens_dev, nseq, Tmax, H, chunk, 0, interleaved, kernel, waves)
        worst = max(worst, check_rows(full, lens, refs, ar.bound_bf16))
        for qb in ar.q_begins(lens, chunk):
            part = run_direct(qkv, lens_dev, nseq, Tmax, H, chunk, qb, interleaved, kernel, waves)
            worst = max(worst, check_rows(part, lens, refs, ar.bound_bf16, qb))
            for s, n in enumerate(lens):
                assert torch.equal(part[s, qb:n], full[s, qb:n]), (kernel, waves, qb, s)
    note("parity_attn.json", f"q_begin.{'.'.join(map(str, lens))}-c{chunk}-{'interleaved' if interleaved else 'plain'}", worst)
    assert worst <= 1.0, worst


def tab_layout(name, row_step, seqs):
    """DitSeqTab rows (q_begin, len, in_row, out_row) and the row counts of the input and output buffers.  row_step 2: the stream
    slots' layout - sequences 2 i and 2 i + 1 interleaved in slot i's 2 cap rows, their new rows interleaved and compact in the
    output; `incremental*`: one stream in place (in_row = s, out_row = 2 T0 + s).  row_step 1: disjoint blocks."""
    tab, Tmax = [], max(n for _, n in seqs)
    if name.startswith("incremental"):
        return [(qb, n, s, 2 * qb + s) for s, (qb, n) in enumerate(seqs)], 2 * Tmax, 2 * Tmax + 4
    if row_step == 2:
        cap, Mn = Tmax + 1, 0
        for i in range(0, len(seqs), 2):
            for sq, (qb, n) in enumerate(seqs[i:i + 2]):
                tab.append((qb, n, 2 * cap * (i // 2) + sq, Mn + sq))
            Mn += 2 * max(n - qb for qb, n in seqs[i:i + 2])
        return tab, 2 * cap * (len(seqs) // 2), Mn + 4
    r_in = r_out = 0
    for qb, n in seqs:
        tab.append((qb, n, r_in, r_out))
        r_in, r_out = r_in + n + 3, r_out + n - qb
    return tab, r_in, r_out + 4


def pack_tab(X, tab, rows_in, row_step):
    """device bf16 [rows_in][3 H 64]: frame t of sequence s at in_row + t row_step; NaN everywhere else"""
    buf = torch.full((rows_in, X[0, 0].numel()), float("nan"))
    for s, (_, n, in_row, _) in enumerate(tab):
        buf[in_row:in_row + n * row_step:row_step] = X[s, :n].reshape(n, -1)
    return buf.to(torch.bfloat16).to(DEV).contiguous()


def expected_tab(base, tab, rows_out, row_step):
    """int16 bits [rows_out][H 64]: query t >= q_begin of sequence s at out_row + (t - q_begin) row_step, the sentinel elsewhere"""
    exp = torch.full((rows_out, base.shape[2] * ar.D), SENTINEL, dtype=torch.int16)
    for s, (qb, n, _, out_row) in enumerate(tab):
        if qb < n:
            exp[out_row:out_row + (n - qb) * row_step:row_step] = base[s, qb:n].reshape(n - qb, -1)
    return exp


@pytest.mark.parametrize("chunk", ar.TAB_CHUNKS)
@pytest.mark.parametrize("name,row_step,seqs", ar.TAB, ids=[t[0] for t in ar.TAB])
def test_dit_attention_tab(name, row_step, seqs, chunk):
    """The per-sequence table form (stream slots): each sequence's own q_begin, length, input and output rows.  Bit-identical to
    fy_debug_dit_attention on the same rows and keys in the same forced form, nothing else written, inside the bound."""
    L, check = hooks()
    lens, H = [n for _, n in seqs], 2
    nseq, Tmax = len(lens), max(lens)
    X, refs = reference(lens, chunk)
    tab, rows_in, rows_out = tab_layout(name, row_step, seqs)
    qkv_tab, qkv = pack_tab(X, tab, rows_in, row_step), pack(X, lens)
    tab_dev = torch.tensor(tab, dtype=torch.int32, device=DEV)
    lens_dev = torch.tensor(lens, dtype=torch.int32, device=DEV)
    worst = 0.0
    for waves in (0, 4, 8):
        base = run_direct(qkv, lens_dev, nseq, Tmax, H, chunk, 0, False, 0, waves)
        worst = max(worst, check_rows(base, lens, refs, ar.bound_bf16))
        out = sentinel(rows_out, H * ar.D)
        check(L.fy_debug_dit_attention_tab(qkv_tab.data_ptr(), out.data_ptr(), tab_dev.data_ptr(), nseq, Tmax, H, chunk, row_step, waves, None))
        torch.cuda.synchronize()
        assert torch.equal(bits(out), expected_tab(base, tab, rows_out, row_step)), waves
    note("parity_attn.json", f"tab.{name}-c{chunk}", worst)
    assert worst <= 1.0, worst


def run_split(hi, lo, lens_dev, nseq, Tmax, H, chunk):
    L, check = hooks()
    oh, ol = sentinel(nseq * Tmax, H * ar.D), sentinel(nseq * Tmax, H * ar.D)
    check(L.fy_debug_dit_attention_split(hi.data_ptr(), lo.data_ptr(), oh.data_ptr(), ol.data_ptr(), lens_dev.data_ptr(), nseq, Tmax, H, chunk, None))
    torch.cuda.synchronize()
    return unpack(oh, nseq), unpack(ol, nseq)


@pytest.mark.parametrize("c", ar.SPLIT, ids=ar.cid)
def test_dit_attention_split_against_float64(c):
    """The fp32-class form on hi + lo planes (workgroups of 4 .. 8 waves over these lengths): out_hi + out_lo against the float64
    attention of hi + lo."""
    nseq, Tmax = len(c.lens), max(c.lens)
    (Xh, Xl), refs = reference(c.lens, c.chunk, "split", c.H)
    lens_dev = torch.tensor(c.lens, dtype=torch.int32, device=DEV)
    oh, ol = run_split(pack(Xh, c.lens), pack(Xl, c.lens), lens_dev, nseq, Tmax, c.H, c.chunk)
    worst = 0.0
    for s, n in enumerate(c.lens):
        assert (oh[s, n:] == SENTINEL_I16).all() and (ol[s, n:] == SENTINEL_I16).all(), f"sequence {s}: a row past {n} was written"
        got = as_float(oh[s, :n]).double() + as_float(ol[s, :n]).double()
        assert torch.isfinite(got).all(), f"sequence {s}: non-finite output"
        o, a = refs[s]
        worst = max(worst, ar.ratio(got, o, ar.bound_split(o, a)))
    print(ar.cid(c), worst)
    note("parity_attn.json", f"split.{ar.cid(c)}", worst)
    assert worst <= 1.0, worst


@pytest.mark.parametrize("chunk", [ar.CHUNK, 7])
@pytest.mark.parametrize("name,row_step,seqs", ar.SPLIT_TAB, ids=[t[0] for t in ar.SPLIT_TAB])
def test_dit_attention_split_tab_equals_split(name, row_step, seqs, chunk):
    """The table form of the split kernel (fp32-class stream slots and incremental chunks): both output planes bit for bit what
    fy_debug_dit_attention_split gives for the same rows and keys (attn.h), nothing else written."""
    L, check = hooks()
    lens, H = [n for _, n in seqs], 2
    nseq, Tmax = len(lens), max(lens)
    (Xh, Xl), _ = reference(lens, chunk, "split", H)
    tab, rows_in, rows_out = tab_layout(name, row_step, seqs)
    lens_dev = torch.tensor(lens, dtype=torch.int32, device=DEV)
    tab_dev = torch.tensor(tab, dtype=torch.int32, device=DEV)
    base_h, base_l = run_split(pack(Xh, lens), pack(Xl, lens), lens_dev, nseq, Tmax, H, chunk)
    qh, ql = pack_tab(Xh, tab, rows_in, row_step), pack_tab(Xl, tab, rows_in, row_step)
    oh, ol = sentinel(rows_out, H * ar.D), sentinel(rows_out, H * ar.D)
    check(L.fy_debug_dit_attention_split_tab(qh.data_ptr(), ql.data_ptr(), oh.data_ptr(), ol.data_ptr(), tab_dev.data_ptr(), nseq, Tmax, H, chunk, row_step, None))
    torch.cuda.synchronize()
    assert torch.equal(bits(oh), expected_tab(base_h, tab, rows_out, row_step))
    assert torch.equal(bits(ol), expected_tab(base_l, tab, rows_out, row_step))


@pytest.mark.parametrize("kernel,waves", [(0, 5), (0, 16), (1, 3), (1, 7), (1, 17), (2, 4), (0, -1)])
def test_hook_refuses_a_form_the_kernel_does_not_have(kernel, waves):
    L, _ = hooks()
    qkv, out, lens_dev = sentinel(32, 3 * 2 * ar.D), sentinel(32, 2 * ar.D), torch.tensor([32], dtype=torch.int32, device=DEV)
    assert L.fy_debug_dit_attention(qkv.data_ptr(), out.data_ptr(), lens_dev.data_ptr(), 1, 32, 2, 0, 0, 0, kernel, waves, None) == -1           # FY_ERR_ARG
    torch.cuda.synchronize()
    assert (bits(out) == SENTINEL_I16).all()
