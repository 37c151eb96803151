"""The edges of the streamed loop (VideoInterpolator.run) in its three modes - the fixed grid, a timeline, a timeline with a shutter: a
writer that raises, a stream without a frame, a stream cut short inside a frame, a writer of another format, a clip of one frame.  What
the loop does then is its failure protocol (ssm_amd.video.PassRing, whose own tests are tests/test_video_ring_cpu.py): the first exception
reaches the caller as it is, nothing is written after it, nothing is left behind in the VideoInterpolator, and nothing hangs.

64 x 96, 4:2:0, 6 frames, synthetic weights, two streams.  One case needs a longer clip: at 60 -> 24 with a 180 degree shutter in 4 samples
the last sample of output k sits at 5 k / 2 + 15 / 16, so 6 frames give two outputs and a writer never sees a third call; the shutter's
failing-writer case reads 11 frames (four outputs)."""
import io
import os
import sys
from fractions import Fraction as Fr

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from video_clips import V, clip_file, clip_payloads  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
H, W, N = 64, 96, 6
# mode -> (the arguments of VideoInterpolator, the clip's rate, the frames the failing-writer case reads)
MODES = {"fixed": (dict(upsample_rate=3), (30, 1), N),
         "timeline": (dict(target_rate=(75, 1)), (30, 1), N),
         "shutter": (dict(target_rate=(24, 1), shutter=Fr(1, 2), shutter_samples=4), (60, 1), 11)}


# Frames written when the stream is cut inside its fourth frame: every pass closed on frames 0 .. 2 is handed over and written before the
# reader's error reaches the caller.  fixed: frame 0 and two passes of one pair, 1 + 3 + 3.  timeline (step 2/5): the passes that frames 1
# and 2 close hold the outputs at 0 .4 .8 and at 1.2 1.6 2.  shutter: frame 1 closes the pass of output 0 (samples at 0 .. 15/16); output
# 1 starts at 5/2, so frame 2 waits for its right neighbour in a pass that never closes.
WRITTEN_BEFORE_THE_CUT = {"fixed": 7, "timeline": 6, "shutter": 1}


class Marker(Exception):
    pass


@pytest.fixture(scope="module")
def model():
    from models.superslomo_r import FullModel
    from ssm_amd.config import load_config, synthetic_weight_overrides
    from ssm_amd.weights import synthetic_state_dict
    cfg = load_config("superslomo_original.ini", synthetic_weight_overrides())
    m = FullModel(cfg)
    m.stage1_model.load_state_dict(synthetic_state_dict(1))
    m.stage2_model.load_state_dict(synthetic_state_dict(2))
    return cfg, m.to(DEV).eval()


def interpolator(model, mode):
    cfg, m = model
    return V().VideoInterpolator(m, cfg, n_streams=2, **MODES[mode][0])


def out_rate(mode):
    kw, rate, _ = MODES[mode]
    return kw.get("target_rate") or V().output_rate(rate, kw["upsample_rate"])


def open_clip(mode, data):
    """(reader of the stream `data`, a writer like it into memory, that memory)."""
    v = V()
    r = v.Y4MReader(io.BytesIO(data))
    sink = io.BytesIO()
    return r, v.Y4MWriter.like(sink, r, rate=out_rate(mode)), sink


def frames_of(sink, fb):
    """The frames of an output stream that may hold none: [n, frame_bytes] uint8."""
    data = sink.getvalue()
    body = data[data.index(b"\n") + 1:]
    rec = len(b"FRAME\n") + fb
    assert len(body) % rec == 0, "the output ends inside a frame record"
    return np.frombuffer(body, np.uint8).reshape(len(body) // rec, rec)[:, len(b"FRAME\n"):]


@pytest.fixture(scope="module")
def full(model):
    """mode -> (the 6-frame clip as a stream, the output of a fresh VideoInterpolator on it); each computed once, on first use."""
    made = {}

    def get(mode):
        if mode not in made:
            data = clip_file(clip_payloads(N, H, W, 0), H, W, rate=MODES[mode][1]).getvalue()
            r, wr, sink = open_clip(mode, data)
            count = interpolator(model, mode).run(r, wr)
            got = frames_of(sink, r.frame_bytes)
            assert count == got.shape[0] == wr.frames_written
            made[mode] = (data, got)
        return made[mode]
    return get


@pytest.mark.parametrize("mode", list(MODES))
def test_a_writer_that_raises(model, full, mode):
    """write_frame raises on its third call: run() raises that exception, two frames were written and no call followed; the same
    VideoInterpolator then gives a good clip the bytes a fresh one gives."""
    rate, n = MODES[mode][1:]
    r, wr, sink = open_clip(mode, clip_file(clip_payloads(n, H, W, 0), H, W, rate=rate).getvalue())
    marker, calls, real = Marker("the writer's third call"), [0], wr.write_frame

    def failing(buf):
        calls[0] += 1
        if calls[0] == 3:
            raise marker
        real(buf)
    wr.write_frame = failing
    vi = interpolator(model, mode)
    with pytest.raises(Marker) as e:
        vi.run(r, wr)
    assert e.value is marker
    assert calls[0] == 3 and wr.frames_written == 2 and frames_of(sink, r.frame_bytes).shape[0] == 2
    data, fresh = full(mode)
    r, wr, sink = open_clip(mode, data)
    assert vi.run(r, wr) == fresh.shape[0]
    assert np.array_equal(frames_of(sink, r.frame_bytes), fresh), "a run that failed left something behind"


@pytest.mark.parametrize("mode", list(MODES))
def test_a_stream_without_a_frame(model, mode):
    v = V()
    r, wr, sink = open_clip(mode, clip_file([], H, W, rate=MODES[mode][1]).getvalue())
    with pytest.raises(v.Y4MError, match="holds no frame"):
        interpolator(model, mode).run(r, wr)
    assert wr.frames_written == 0 and frames_of(sink, r.frame_bytes).shape[0] == 0


@pytest.mark.parametrize("mode", list(MODES))
def test_a_stream_cut_inside_its_fourth_frame(model, full, mode):
    v = V()
    data, fresh = full(mode)
    fb = v.frame_bytes(H, W, 0)
    cut = data.index(b"\n") + 1 + 3 * (len(b"FRAME\n") + fb) + len(b"FRAME\n") + fb // 2
    r, wr, sink = open_clip(mode, data[:cut])
    with pytest.raises(v.Y4MError, match="truncated"):
        interpolator(model, mode).run(r, wr)
    got = frames_of(sink, fb)
    print("%s: %d of %d frames written before the cut" % (mode, got.shape[0], fresh.shape[0]))
    assert got.shape[0] == wr.frames_written == WRITTEN_BEFORE_THE_CUT[mode]
    assert np.array_equal(got, fresh[:got.shape[0]]), "what was written before the cut is a prefix of the whole clip's output"


@pytest.mark.parametrize("mode", list(MODES))
def test_a_writer_of_another_frame_size(model, full, mode):
    v = V()
    r = v.Y4MReader(io.BytesIO(full(mode)[0]))
    sink = io.BytesIO()
    wr = v.Y4MWriter(sink, W + 2, H, rate=out_rate(mode), aspect=(1, 1))
    with pytest.raises(ValueError, match="disagree") as e:
        interpolator(model, mode).run(r, wr)
    assert not isinstance(e.value, v.Y4MError)
    assert r.frames_read == 0, "refused before anything is read"
    assert wr.frames_written == 0


@pytest.mark.parametrize("mode", list(MODES))
def test_a_clip_of_one_frame(model, mode):
    v = V()
    kw, rate, _ = MODES[mode]
    payloads = clip_payloads(1, H, W, 0)
    r, wr, sink = open_clip(mode, clip_file(payloads, H, W, rate=rate).getvalue())
    count = interpolator(model, mode).run(r, wr)
    got = frames_of(sink, r.frame_bytes)
    assert count == got.shape[0] == wr.frames_written
    if mode == "shutter":
        assert count == 0 == v.Timeline(Fr(5, 2), shutter=kw["shutter"], samples=kw["shutter_samples"]).n_outputs(1)
    else:
        assert count == 1 and np.array_equal(got[0], payloads[0]), "the frame's own bytes"
