"""The layout of a packed flow call (FY_PACKED, include/fy_cosy3.h) as `flow.packed_rows` states it: hand-checked inputs.  The C
side is held to the same function on the GPU (tests/test_flow_packed_gpu.py, through `FlowEngine.last_rows`)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_packed_rows_hand_checked():
    from fangyan_tts_amd.flow import packed_rows
    assert packed_rows([7]) == ([0, 7], 14)                               # one utterance: its two sequences back to back
    assert packed_rows([50, 50, 50]) == ([0, 50, 100, 150, 200, 250], 300)      # equal lengths: the padded layout itself
    assert packed_rows([2, 400, 34]) == ([0, 2, 4, 404, 804, 838], 872)
    assert packed_rows((2, 400, 34))[1] == 2 * (2 + 400 + 34)
    off, Mp = packed_rows([60, 48, 26, 2])
    assert off == [0, 60, 120, 168, 216, 242, 268, 270] and Mp == 272


@pytest.mark.parametrize("T", [[0], [5, 0, 3], [4, -2]])
def test_packed_rows_rejects_an_empty_sequence(T):
    from fangyan_tts_amd.flow import packed_rows
    with pytest.raises(ValueError):
        packed_rows(T)


def test_flag_and_getter_are_declared():
    from fangyan_tts_amd import _lib
    with open(os.path.join(ROOT, "include", "fy_cosy3.h")) as fh:
        hdr = fh.read()
    m = re.search(r"#define\s+FY_PACKED\s+(\d+)u", hdr)
    assert m and int(m.group(1)) == _lib.FY_PACKED == 32
    flags = [_lib.FY_PRECISE, _lib.FY_DIRECT, _lib.FY_STREAMING, _lib.FY_NO_FINALIZE, _lib.FY_INCREMENTAL, _lib.FY_PACKED]
    assert len({f for f in flags}) == 6 and all(f & (f - 1) == 0 for f in flags)      # six distinct bits
    assert re.search(r"int64_t\s+fy_flow_last_rows\(const fy_flow\*\s*f\);", hdr)
