"""Flow stream slots without a GPU: the chunk schedule as a pure function (fangyan_tts_amd.flow.stream_chunk_plan / stream_poll_plan)
against the chunk boundaries the reference produced (tests/golden/stream_{tiny,full}.npz), and the header's new entries."""
import os
import re

import numpy as np
import pytest

from fangyan_tts_amd.flow import stream_chunk_plan, stream_poll_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UP = 480                                                  # samples per mel frame


def chunk_samples(plan, look=3):
    """Samples each chunk yields: the vocoder holds 8 frames back until the final pass (cli/model.py:416-441)."""
    out, done = [], 0
    for n_in, _, fin in plan:
        end = UP * (2 * n_in if fin else 2 * (n_in - look) - 8)
        out.append(end - done)
        done = end
    return out


@pytest.mark.parametrize("tag,ctag,p_flow", [("tiny", "40_6_0_12", 12), ("full", "8_8_0_25", 25)])
def test_chunk_plan_gives_the_reference_boundaries(tag, ctag, p_flow):
    f = np.load(os.path.join(ROOT, "tests", "golden", f"stream_{tag}.npz"))
    n = len(f[f"e2e.c{ctag}.tokens"])
    assert chunk_samples(stream_chunk_plan(n, p_flow)) == f[f"e2e.c{ctag}.chunk_samples"].tolist()


def test_chunk_plan_by_hand():
    assert stream_chunk_plan(85, 12) == [(41, 0, False), (66, 38, False), (85, 63, True)]
    assert stream_chunk_plan(60, 25) == [(28, 0, False), (53, 25, False), (60, 50, True)]
    assert stream_chunk_plan(10, 50) == [(10, 0, True)]                      # shorter than the first hop: the final pass only
    assert stream_chunk_plan(28, 0) == [(28, 0, False), (28, 25, True)]
    for n, p in ((103, 50), (77, 13), (300, 40)):
        for n_in, _, fin in stream_chunk_plan(n, p):
            assert fin or (2 * (p + n_in - 3)) % 50 == 0                    # every streaming call ends on a chunk-mask boundary


@pytest.mark.parametrize("per_poll", [25, 8, 60])
def test_every_stream_keeps_its_own_boundaries(per_poll):
    n_tokens, n_prompt = [85, 60, 10, 131, 28], [12, 25, 50, 40, 0]
    polls = stream_poll_plan(n_tokens, n_prompt, tokens_per_poll=per_poll)
    for i, (n, p) in enumerate(zip(n_tokens, n_prompt)):
        mine = [(n_in, off, fin) for poll in polls for (s, n_in, off, fin) in poll if s == i]
        assert mine == stream_chunk_plan(n, p), i
    for poll in polls:                                                       # at most one entry per stream and poll
        assert len({s for s, *_ in poll}) == len(poll)


def test_header_declares_the_stream_slot_entries():
    src = open(os.path.join(ROOT, "include", "fy_cosy3.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = set(re.findall(r"\b(fy_[a-z0-9_]+)\s*\(", src))
    for want in ("fy_flow_streams_open", "fy_flow_streams_close", "fy_flow_streams_bytes", "fy_flow_stream_slot_reset",
                 "fy_flow_stream_slot_rows", "fy_flow_infer_streams"):
        assert want in names, want
    assert {"fy_flow_infer", "fy_flow_stream_reset", "fy_flow_stream_rows"} <= names
