"""HiFT stream slots without a GPU: the sample count of an incremental vocoder call as a pure function
(fangyan_tts_amd.hift.stream_new_samples) against the chunk lengths the reference produced (tests/golden/stream_{tiny,full}.npz),
and the header's new entries."""
import os
import re

import numpy as np
import pytest

from fangyan_tts_amd.flow import stream_chunk_plan
from fangyan_tts_amd.hift import stream_new_samples

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UP = 480                                                  # samples per mel frame


def chunk_samples(plan, look=3):
    """Samples each vocoder call of a stream brings: the mel so far holds 2 * (tokens - look-ahead) frames until the final pass."""
    out, done = [], 0
    for n_in, _, fin in plan:
        frames = 2 * (n_in if fin else n_in - look)
        out.append(stream_new_samples(frames, fin, done))
        done += out[-1]
    return out


@pytest.mark.parametrize("tag,ctag,p_flow", [("tiny", "40_6_0_12", 12), ("full", "8_8_0_25", 25)])
def test_new_samples_give_the_reference_chunks(tag, ctag, p_flow):
    f = np.load(os.path.join(ROOT, "tests", "golden", f"stream_{tag}.npz"))
    n = len(f[f"e2e.c{ctag}.tokens"])
    want = f[f"e2e.c{ctag}.chunk_samples"].tolist()
    assert chunk_samples(stream_chunk_plan(n, p_flow)) == want
    assert sum(want) == UP * 2 * n


def test_new_samples_by_hand():
    assert stream_new_samples(80, False, 0) == UP * 72                       # a first chunk: 8 frames held back
    assert stream_new_samples(130, False, UP * 72) == UP * 50                # the next one: the 50 new frames
    assert stream_new_samples(150, True, UP * 122) == UP * 28                # the final call releases the 8 frames held back
    assert stream_new_samples(95, True, 0) == UP * 95                        # a stream whose only call is a finalize
    assert stream_new_samples(60, False, 0) == UP * 52                       # a chunk after a reset: counted from nothing again
    assert stream_new_samples(10, False, 0, up=120) == 240                   # another up-sampling factor


def test_header_declares_the_stream_slot_entries():
    src = open(os.path.join(ROOT, "include", "fy_cosy3.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = set(re.findall(r"\b(fy_[a-z0-9_]+)\s*\(", src))
    for want in ("fy_hift_streams_open", "fy_hift_streams_close", "fy_hift_streams_bytes", "fy_hift_stream_slot_reset",
                 "fy_hift_stream_slot_samples", "fy_hift_stream_slot_window", "fy_hift_infer_streams"):
        assert want in names, want
    assert {"fy_hift_infer", "fy_hift_stream_reset", "fy_hift_stream_samples", "fy_hift_stream_window"} <= names
