"""No-GPU checks of the scene cuts of the streamed video path (VideoInterpolator(scene_cut=)): the host yardstick of
ssm_luma_sad_fwd against a plain Python sum; the decision (ssm_amd.video.SceneCuts) on hand-written sums; the texts parse_scene_cut takes
and refuses; the entry point declared, exported and bound; the refusals beside a shutter; the bookkeeping the loop adds without a GPU in
it (sad_runs, PassPlanner.closed_index, rows decided on the writer thread); and the clip of the GPU tests (tests/video_cut_clips.py)
through the yardstick: at the threshold both test files use, pair (4, 5) is a cut and no other pair is, with a factor of 2 to spare."""
import os
import re
import subprocess
import sys
from fractions import Fraction as Fr

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import video_cut_clips as C  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "ssm_luma_sad_fwd"


def cfg():
    from ssm_amd.config import load_config, synthetic_weight_overrides
    return load_config("superslomo_original.ini", synthetic_weight_overrides())


def test_host_yardstick_is_the_plain_sum():
    from ssm_amd.video import luma_sad_host
    rng = np.random.RandomState(2)
    ya, yb = rng.randint(0, 256, size=(2, 3, 5)).astype(np.uint8), rng.randint(0, 256, size=(2, 3, 5)).astype(np.uint8)
    ya[0, 0, 0], yb[0, 0, 0], ya[1, 2, 4], yb[1, 2, 4] = 0, 255, 255, 0          # both signs at full range: no uint8 wrap-around
    want = [sum(abs(int(ya[n, y, x]) - int(yb[n, y, x])) for y in range(3) for x in range(5)) for n in range(2)]
    got = luma_sad_host(ya, yb)
    assert got.dtype == np.uint64 and got.shape == (2,) and got.tolist() == want
    assert luma_sad_host(ya, ya).tolist() == [0, 0]
    assert luma_sad_host(np.zeros((1, 3, 5), np.uint8), np.full((1, 3, 5), 255, np.uint8)).tolist() == [255 * 15]


def test_scene_cuts_on_hand_written_sums():
    from ssm_amd.video import SceneCuts
    px = 100
    sc = SceneCuts(Fr(1, 10))
    # the first pair: m_prev = 0, so its score is its own mean difference: m = 20 -> 20/255 < 1/10
    assert sc.feed(2000, px) == (False, Fr(20, 255))
    # steady high difference: m = 200 after m = 200 scores 0, however large m is - but the step up to it is a spike
    sc = SceneCuts(Fr(1, 10))
    assert sc.feed(20000, px) == (True, Fr(200, 255))          # first pair at m = 200: nothing damps it
    assert sc.feed(20000, px) == (False, Fr(0))
    assert sc.feed(20100, px) == (False, Fr(1, 255))
    assert sc.feed(19900, px) == (False, Fr(2, 255))
    # a spike: m = 10, 10, 150, 10 - the spike is a cut (min(150, 140) = 140), the way back is damped by the small m (min(10, 140) = 10)
    sc = SceneCuts(Fr(1, 10))
    got = [sc.feed(s, px) for s in (1000, 1000, 15000, 1000)]
    assert got == [(False, Fr(10, 255)), (False, Fr(0)), (True, Fr(140, 255)), (False, Fr(10, 255))]
    # score == threshold is a cut; one unit of the sum below is not
    sc = SceneCuts(Fr(51, 255))
    assert sc.feed(5100, px) == (True, Fr(51, 255))
    sc = SceneCuts(Fr(51, 255))
    assert sc.feed(5099, px) == (False, Fr(5099, 25500))
    # exact for sums beyond 2^53 and numpy integers
    sc = SceneCuts(1)
    assert sc.feed(np.uint64(255 * (1 << 55)), 1 << 55) == (True, Fr(1))
    assert sc.feed(np.uint64(255 * (1 << 55) - 1), 1 << 55) == (False, Fr(1, 255 * (1 << 55)))


def test_parse_scene_cut():
    from ssm_amd.video import SceneCuts, parse_scene_cut
    assert parse_scene_cut("0.1") == Fr(1, 10) == parse_scene_cut("1/10") == parse_scene_cut(" 1/10 ") == parse_scene_cut(Fr(1, 10))
    assert parse_scene_cut("1") == 1 and parse_scene_cut(0.5) == Fr(1, 2) and parse_scene_cut("3e-2") == Fr(3, 100)
    for bad in ("0", "-0.1", "1.01", "3/2", 0, -1):
        with pytest.raises(ValueError, match="above 0 and at most at 1"):
            parse_scene_cut(bad)
    for bad in ("", "x", "1/0", "0.1.2", None, "10%"):
        with pytest.raises(ValueError, match="written as a decimal or a fraction"):
            parse_scene_cut(bad)
    with pytest.raises(ValueError, match="above 0"):
        SceneCuts(0)
    assert SceneCuts("1/4").threshold == Fr(1, 4)


def test_entry_point_is_declared_exported_and_bound():
    import ctypes
    from ssm_amd import hipbind as hb
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ssm_hip.h")).read(), flags=re.S)
    m = re.search(r"int\s+%s\s*\(([^)]*)\)" % ENTRY, src)
    assert m, "include/ssm_hip.h does not declare %s" % ENTRY
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["const unsigned char *a", "const unsigned char *b", "long long stride_a", "long long stride_b", "int N", "int H", "int W",
                    "unsigned long long *sums", "void *stream"]
    out = subprocess.run(["nm", "-D", "--defined-only", hb.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert any(ln.split()[-1] == ENTRY and " T " in ln for ln in out.splitlines()), "libssm_hip.so does not export %s" % ENTRY
    res, argtypes = hb.SIGNATURES[ENTRY]
    assert res is ctypes.c_int and len(argtypes) == len(args) and argtypes[2:4] == [ctypes.c_longlong, ctypes.c_longlong]
    assert argtypes[4:7] == [ctypes.c_int] * 3 and argtypes[7] is ctypes.c_void_p
    assert hasattr(hb.load(), ENTRY)


def test_scene_cut_beside_a_shutter_is_refused_by_name():
    import interpolate_video
    from ssm_amd.video import VideoInterpolator
    c = cfg()
    with pytest.raises(ValueError, match="scene_cut together with shutter"):
        VideoInterpolator(None, c, speed=1, shutter=Fr(1, 2), scene_cut=Fr(1, 10))
    with pytest.raises(ValueError, match="scene_cut together with shutter"):
        VideoInterpolator(None, c, target_rate=(24, 1), shutter="1/2", shutter_samples=1, scene_cut="0.1")
    with pytest.raises(ValueError, match="above 0 and at most at 1"):
        VideoInterpolator(None, c, scene_cut=2)
    vi = VideoInterpolator(None, c, scene_cut="1/10")
    assert vi.scene_cut == Fr(1, 10) and vi.cuts == [] and VideoInterpolator(None, c).scene_cut is None
    base = ["-c", "x.ini", "--expt", "e", "--log", "l", "--input", "-", "--output", "-"]
    assert interpolate_video.getargs(base).scene_cut is None, "the option has no default value"
    assert interpolate_video.getargs(base + ["--scene_cut", "1/10"]).scene_cut == Fr(1, 10)
    assert interpolate_video.getargs(base + ["--scene_cut", "0.25", "--fps", "60"]).scene_cut == Fr(1, 4)
    for bad in (["--scene_cut", "0.1", "--fps", "24", "--shutter", "180"], ["--scene_cut", "0"], ["--scene_cut", "x"], ["--scene_cut"]):
        with pytest.raises(SystemExit):
            interpolate_video.getargs(base + bad)


def test_refusal_on_the_command_line_names_the_two_flags(capsys):
    import interpolate_video
    with pytest.raises(SystemExit):
        interpolate_video.getargs(["-c", "x.ini", "--expt", "e", "--log", "l", "--input", "-", "--output", "-", "--speed", "1/2", "--shutter", "180",
                                   "--scene_cut", "0.1"])
    err = capsys.readouterr().err
    assert "--scene_cut does not go together with --shutter" in err


def test_sad_runs():
    from ssm_amd.video import sad_runs
    assert sad_runs([0], [1]) == [(0, 1)]
    assert sad_runs([0, 1, 2], [1, 2, 3]) == [(0, 3)]                  # the fixed grid: every pair follows the one before
    assert sad_runs([0, 3], [1, 4]) == [(0, 2)]                        # two pairs always make one run, whatever lies between them
    assert sad_runs([1, 3], [2, 4]) == [(0, 2)]
    assert sad_runs([0, 1, 3], [1, 2, 4]) == [(0, 2), (2, 1)]          # a skipped pair inside a pass of three
    assert sad_runs([1, 3, 5, 6], [2, 4, 6, 7]) == [(0, 3), (3, 1)]
    assert sad_runs([], []) == []


def test_planner_names_the_pairs_of_the_pass_it_closed():
    from ssm_amd.video import PassPlanner, Timeline
    tl = Timeline(Fr(6, 5))          # taus 0 6/5 12/5 18/5 24/5 6: pairs 1, 2, 3 and 4 get a frame, pairs 0, 5 and 6 none
    plan = PassPlanner(tl, 2, 6)
    seen = []
    for _ in range(8):
        closed = plan.frame()
        if closed is not None:
            seen.append((list(plan.closed_index), len(closed[1])))
    closed = plan.end()
    seen.append((list(plan.closed_index), len(closed[1])))
    assert [i for idx, _ in seen for i in idx] == [1, 2, 3, 4] and all(len(idx) == m for idx, m in seen)


def test_ring_calls_a_callable_for_its_rows_after_the_event():
    from ssm_amd.video import PassRing
    log = []

    class Event:
        def synchronize(self):
            log.append("sync")

    class Writer:
        def write_frame(self, buf):
            log.append(buf)

    def rows():
        log.append("rows")
        yield "a"
        yield "b"
        log.append("end")

    ring = PassRing(1, Writer())
    r = ring.take(timeout=10)
    ring.hand(r, Event(), rows)
    assert ring.take(timeout=10) == r
    ring.close()
    assert log == ["sync", "rows", "a", "b", "end"]


def test_rows_of_a_pass_under_cuts():
    """PairOptions.written, the writer thread's callable, without a GPU: two passes of two pairs at upsample_rate 4, the cut in the first
    pair of the second pass - its left frame is the one the first pass carried over."""
    from ssm_amd.video import C444, LIMITED, BT601, Clip, PairOptions, VideoInterpolator
    vi = VideoInterpolator(None, cfg(), upsample_rate=4, pairs_per_batch=2, scene_cut=Fr(1, 10))
    opt = PairOptions(vi, Clip(1, 10, C444, BT601, LIMITED), vi.scene_cut)          # a luma plane of 10 pixels
    assert opt.pixels == 10 and opt.lead == 1 and opt.paste is None
    carried = opt.carried = np.array([0], np.uint8)
    frames = [np.array([10 + i], np.uint8) for i in range(5)]          # input frames 0 .. 4 as one-byte payloads; `carried` starts as frame 0
    carried[:] = frames[0]
    synth = {(i, s): np.array([100 + 10 * i + s], np.uint8) for i in range(4) for s in (1, 2, 3)}
    got = []
    for i0, sums in ((0, [0, 5]), (2, [1500, 5])):
        pairs = [(i0 + p, frames[i0 + p] if p else None, frames[i0 + p + 1]) for p in range(2)]
        order = []
        for p in range(2):
            order += [(synth[(i0 + p, s)], (p, Fr(s, 4))) for s in (1, 2, 3)] + [(frames[i0 + p + 1], None)]
        got += [int(b[0]) for b in opt.written([i for i, _, _ in pairs], np.array(sums, np.uint64), None, pairs, order)]
        assert int(carried[0]) == 10 + i0 + 2
    assert got == [101, 102, 103, 11, 111, 112, 113, 12,          # pairs 0 and 1 as synthesised
                   12, 13, 13, 13, 131, 132, 133, 14]            # pair 2 is the cut: frame 2 at t = 1/4, frame 3 at t = 1/2 and 3/4
    assert vi.cuts == [(2, Fr(150 - Fr(1, 2), 255))]


@pytest.mark.parametrize("h,w", C.SIZES)
def test_the_clip_of_the_gpu_tests_has_one_cut_with_room(h, w):
    payloads = C.cut_clip(h, w)
    assert payloads.shape[0] == C.N_FRAMES == 10 and C.CUT == 4
    y = C.luma(payloads, h, w)
    assert y.min() >= 16 and y.max() <= 235
    scores = C.pair_scores(payloads, h, w)
    assert [i for i, cut, _ in scores if cut] == [C.CUT], scores
    cut = scores[C.CUT][2]
    rest = max(s for i, _, s in scores if i != C.CUT)
    print("%dx%d: cut %.4f, largest other score %.4f, threshold %s" % (h, w, float(cut), float(rest), C.THRESHOLD))
    assert rest > 0, "the scenes move"
    assert 2 * rest <= C.THRESHOLD and 2 * C.THRESHOLD <= cut, (float(rest), float(cut))
    # the timeline of the GPU test (30 -> 75, step 2/5) runs every pair, so it feeds the same pairs in the same order
    from ssm_amd.video import Timeline
    tl = Timeline(Fr(2, 5))
    assert all(tl.count(i) > 0 for i in range(C.N_FRAMES - 1))
    assert [t < Fr(1, 2) for t in tl.times(C.CUT)] == [True, False], "the cut pair gets a frame on either side of its middle"
