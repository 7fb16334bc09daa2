"""The direct attention tests can fail, and their bound is not tuned on the kernels: for every case of tests/test_attention_gpu.py

* a reference whose mask is off by ONE key - the sequence end at len - 1, the chunk limit moved by +1 or by -1 - leaves the
  case's bound by a factor >= 4 in some element (a condition on the chosen inputs: a case that cannot reach it is changed,
  not the factor);
* a NumPy fp32 emulation of the bf16 kernels' rounding (probabilities rounded to bf16 tile by tile, both denominators, both
  tile sizes) stays within 1.0 of the bf16 bound.
"""
import pytest
import torch

import attn_ref as ar

FACTOR = 4.0


def _cases():
    cs = list(ar.DIRECT) + list(ar.SPLIT)
    cs += [ar.Case(l, c, "default", 2) for l, c, _ in ar.QBEGIN]
    cs += [ar.Case([n for _, n in seqs], c, "default", 2) for _, _, seqs in ar.TAB for c in ar.TAB_CHUNKS]
    cs += [ar.Case([n for _, n in seqs], c, "split", 2) for _, _, seqs in ar.SPLIT_TAB for c in (ar.CHUNK, 7)]
    seen, out = set(), []
    for c in cs:
        if ar.cid(c) not in seen:
            seen.add(ar.cid(c))
            out.append(c)
    return out


CASES = _cases()


def _inputs(c):
    if c.mode == "split":
        hi, lo = ar.inputs_split(c.lens, c.H)
        return hi.double() + lo.double(), ar.bound_split
    return ar.inputs(c.lens, c.mode, c.H), ar.bound_bf16


@pytest.mark.parametrize("c", CASES, ids=ar.cid)
def test_one_key_mutants_leave_the_bound(c):
    X, bound = _inputs(c)
    true = ar.ref_batch(X, c.lens, c.chunk)
    mutants = {"len-1": dict(len_shift=-1)}
    if c.chunk > 0 and c.chunk < max(c.lens):                       # a chunk boundary inside some sequence
        mutants.update({"lim+1": dict(lim_shift=1), "lim-1": dict(lim_shift=-1)})
    for name, shifts in mutants.items():
        worst = 0.0
        for s, n in enumerate(c.lens):
            if n < 2:
                continue                                            # (len - 1 would leave a query without keys)
            om, _ = ar.ref(X[s, :, 0], X[s, :, 1], X[s, :, 2], n, c.chunk, ar.visible(n, c.chunk, **shifts))
            o, a = true[s]
            worst = max(worst, ar.ratio(om, o, bound(o, a)))
        assert worst >= FACTOR, (name, worst)


@pytest.mark.parametrize("c", [c for c in CASES if c.mode != "split"], ids=ar.cid)
def test_bf16_emulation_stays_inside_the_bound(c):
    X, bound = _inputs(c)
    true = ar.ref_batch(X, c.lens, c.chunk)
    worst = 0.0
    for tile, sum_bf16 in ((32, True), (64, False)):                # the round-5 kernel's half tiles, the round-2 kernel's tiles
        for s, n in enumerate(c.lens):
            got = ar.emulate(X[s, :, 0], X[s, :, 1], X[s, :, 2], n, c.chunk, tile, sum_bf16)
            assert torch.isfinite(got).all()
            o, a = true[s]
            worst = max(worst, ar.ratio(got, o, bound(o, a)))
    assert worst <= 1.0, worst
