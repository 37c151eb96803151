"""Letterboxed clips through the streamed loop: VideoInterpolator(active=) on the clip of tests/video_active_clips.py - the
64 x 96 picture clip C of the streamed tests inside a 96 x 112 frame whose bottom bar carries a subtitle that changes every frame -
against the same run on C alone, byte for byte inside the rectangle, and against the input frame the rule names outside it: the left
frame of the pair at t < 1/2, else the right one.  Both runs get the matrix explicitly."""
import io
import os
import sys
from fractions import Fraction as Fr

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from video_active_clips import FH, FW, H, RECT, W, boxed, letterboxed, picture_clip  # noqa: E402
from video_clips import V, frames_of, synthetic_model, y4m  # noqa: E402
from video_cut_clips import CUT, THRESHOLD, cut_clip  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
MATRIX = 0          # BT601, said to both runs: the frame's height and the picture's would give the same one here, but the test does not rest on it


@pytest.fixture(scope="module")
def model():
    return synthetic_model(DEV)


def run(m, cfg, payloads, h, w, tag, **kw):
    """The clip through VideoInterpolator(matrix=MATRIX, **kw): (the frames written, the interpolator)."""
    v = V()
    r = v.Y4MReader(y4m(payloads, h, w, tag), extended=True)
    sink = io.BytesIO()
    wr = v.Y4MWriter.like(sink, r, rate=kw.get("target_rate") or r.rate)
    vi = v.VideoInterpolator(m, cfg, matrix=MATRIX, **kw)
    count = vi.run(r, wr)
    assert count == wr.frames_written
    return frames_of(sink.getvalue()), vi


_alone = {}


def alone(m, cfg, tag, **kw):
    """The run on the picture clip alone, once per format and options."""
    key = (tag, tuple(sorted((k, str(x)) for k, x in kw.items())))
    if key not in _alone:
        _alone[key] = run(m, cfg, picture_clip(tag), H, W, tag, **kw)
    return _alone[key]


def where(vi, n, count):
    """[(i, t)] of every output of an n-frame clip: the pair's left frame and the exact time; t = 0 is input frame i itself."""
    if vi.timed:
        return vi.timeline((240, 1)).outputs(n)
    return [(k // vi.rate, Fr(k % vi.rate, vi.rate)) for k in range(count)]


def check(got, vi, clip, want, tag, rect=RECT):
    """Inside the rectangle the run on the picture alone; outside it the input frame of the rule; an input frame is its own bytes."""
    v = V()
    layout, bits = v.EXTENDED_TAGS[tag]
    assert got.shape[0] == want.shape[0] and got.shape[1] == clip.shape[1]
    assert np.array_equal(v.cut_window_host(got, FH, FW, layout, bits, rect), want), "the picture is the run on the cropped clip"
    at = where(vi, clip.shape[0], got.shape[0])
    assert len(at) == got.shape[0]
    blank = np.zeros((1, want.shape[1]), np.uint8)
    synthesised = 0
    for k, (i, t) in enumerate(at):
        if t == 0:
            assert np.array_equal(got[k], clip[i]), "an input frame is its own bytes, whole"
            continue
        synthesised += 1
        near = clip[i] if t < Fr(1, 2) else clip[i + 1]
        bars = lambda x: v.paste_window_host(blank, x[None], FH, FW, layout, bits, rect)          # noqa: E731
        assert np.array_equal(bars(got[k]), bars(near)), "output %d at t = %s of pair %d: the bars of the %s frame" % (k, t, i, "left" if t < Fr(1, 2) else "right")
    assert synthesised


@pytest.mark.parametrize("kw", [dict(upsample_rate=2), dict(upsample_rate=3), dict(target_rate=(600, 1))], ids=["rate2", "rate3", "fps"])
@pytest.mark.parametrize("tag", ["420jpeg", "422p10"])
def test_the_picture_is_the_cropped_run_and_the_bars_are_the_nearer_input_frames(model, tag, kw):
    cfg, m = model
    clip, _ = letterboxed(tag)
    got, vi = run(m, cfg, clip, FH, FW, tag, active=RECT, **kw)
    assert vi.active == RECT and vi.active_excess == [] and "as given" in vi.active_note
    want, _ = alone(m, cfg, tag, **kw)
    check(got, vi, clip, want, tag)


def test_coarse_flow_runs_on_the_windows_canvas(model):
    cfg, m = model
    clip, _ = letterboxed("420jpeg")
    got, vi = run(m, cfg, clip, FH, FW, "420jpeg", active="96:64:8:16", upsample_rate=2, flow_scale=2)
    check(got, vi, clip, alone(m, cfg, "420jpeg", upsample_rate=2, flow_scale=2)[0], "420jpeg")


@pytest.mark.parametrize("kw", [dict(upsample_rate=3), dict(target_rate=(600, 1))], ids=["rate3", "fps"])
def test_scene_cuts_are_those_of_the_picture_and_pass_whole_input_frames(model, kw):
    """A cut in the middle of the picture clip: its pair's outputs are whole input frames - which the rule for the bars gives as well - and
    the pairs beside it are pasted; the sums, and so the cuts and their scores, are the cropped clip's."""
    cfg, m = model
    picture = cut_clip(H, W)[CUT - 2:CUT + 4]          # six frames of the scene-cut tests' clip, the cut between frames 2 and 3
    clip = boxed(picture, "420jpeg")
    got, vi = run(m, cfg, clip, FH, FW, "420jpeg", active=RECT, scene_cut=THRESHOLD, **kw)
    want, ref = run(m, cfg, picture, H, W, "420jpeg", scene_cut=THRESHOLD, **kw)
    assert vi.cuts == ref.cuts and [i for i, _ in vi.cuts] == [2]
    check(got, vi, clip, want, "420jpeg")
    at = where(vi, 6, got.shape[0])
    for k, (i, t) in enumerate(at):
        if i == 2 and t:
            assert np.array_equal(got[k], clip[2] if t < Fr(1, 2) else clip[3]), "a cut pair's frames are whole input frames"


def test_auto_finds_the_rectangle(model):
    cfg, m = model
    for tag in ("420jpeg", "422p10"):
        clip, _ = letterboxed(tag)
        got, vi = run(m, cfg, clip, FH, FW, tag, active="auto", upsample_rate=2)
        assert vi.active == RECT and vi.active_excess == [] and "96:64:8:16" in vi.active_note
        check(got, vi, clip, alone(m, cfg, tag, upsample_rate=2)[0], tag)


def test_whole_frame_fallbacks_write_what_the_run_without_the_option_writes(model):
    cfg, m = model
    tag = "420jpeg"
    layout, bits = V().EXTENDED_TAGS[tag]
    clip, picture = letterboxed(tag, 4)
    plain, _ = run(m, cfg, clip, FH, FW, tag, upsample_rate=2)
    got, vi = run(m, cfg, clip, FH, FW, tag, upsample_rate=2, active=(FW, FH, 0, 0))
    assert vi.active is None and vi.active_note == "the active area is the whole frame" and np.array_equal(got, plain)
    # an all-black probe: the first two frames hold nothing above the limit
    dark = clip.copy()
    V().split_planes(dark[:2], FH, FW, layout, bits)[0][...] = 16
    plain_dark, _ = run(m, cfg, dark, FH, FW, tag, upsample_rate=2)
    got, vi = run(m, cfg, dark, FH, FW, tag, upsample_rate=2, active="auto", active_probe=2)
    assert vi.active is None and vi.active_note == "no active row or column in the 2 probed frames" and np.array_equal(got, plain_dark)
    # a clip without bars
    full = picture_clip(tag, 4)
    plain_full, _ = run(m, cfg, full, H, W, tag, upsample_rate=2)
    got, vi = run(m, cfg, full, H, W, tag, upsample_rate=2, active="auto")
    assert vi.active is None and vi.active_note == "the active area is the whole frame" and np.array_equal(got, plain_full)


def test_a_later_frame_outside_the_rectangle_is_reported_and_changes_nothing(model):
    cfg, m = model
    tag = "420jpeg"
    clip, _ = letterboxed(tag, bright=(4,))          # frame 4's subtitle is a white caption: 6 active rows in the bottom bar
    want = alone(m, cfg, tag, upsample_rate=2)[0]
    for kw in (dict(active="auto", active_probe=3), dict(active=RECT)):
        got, vi = run(m, cfg, clip, FH, FW, tag, upsample_rate=2, **kw)
        assert vi.active == RECT
        assert vi.active_excess == [(4, 6, 0)], "rows 84 .. 89 lie outside; the caption's columns 36 .. 75 are the picture's own"
        check(got, vi, clip, want, tag)


def test_the_output_does_not_depend_on_the_probe_or_the_chunk(model):
    cfg, m = model
    tag = "420jpeg"
    v = V()
    clip, _ = letterboxed(tag, 7, bright=(5,))
    runs = [run(m, cfg, clip, FH, FW, tag, upsample_rate=2, active="auto", active_probe=p) for p in (2, 4, 5)]          # the caption is behind each
    runs.append(run(m, cfg, clip, FH, FW, tag, upsample_rate=2, active=RECT))
    assert all(vi.active == RECT for _, vi in runs), "the rectangle is the same (tests/test_video_active_cpu.py: two frames give it)"
    assert all(np.array_equal(runs[0][0], out) for out, _ in runs[1:])
    assert [vi.active_excess for _, vi in runs] == [[(5, 6, 0)]] * 3 + [[(5, 6, 0)]]
    # the source alone, at three chunk sizes: the frames as they are, the same rectangle, the same excess
    for chunk in (1, 3, 8):
        for active, probe in ((("auto", None, v.ACTIVE_FRAC), 2), (RECT, 48)):
            src = v.ActiveSource(v.Y4MReader(y4m(clip, FH, FW, tag), extended=True), DEV, active, probe, frames_per_chunk=chunk)
            assert src.decide() == RECT
            buf, frames = np.empty(src.frame_bytes, np.uint8), []
            while src.read_frame_into(buf):
                frames.append(buf.copy())
            assert np.array_equal(np.stack(frames), clip) and src.frames_read == 7
            assert src.excess == [(5, 6, 0)], (chunk, active, src.excess)
