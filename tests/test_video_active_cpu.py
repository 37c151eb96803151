"""Letterboxed clips without a GPU: the definition in numpy (active_counts_host, ActiveArea, active_area_host), the window
copies (cut_window_host, paste_window_host), parse_active, the option refusals of VideoInterpolator and the command line, and the
refusals of ssm_luma_counts_fwd and ssm_window_cut_fwd through the library as tests/test_cabi_cpu.py loads it.

The letterboxed clip of tests/video_active_clips.py, which the streamed GPU tests run, must give its own rectangle under the defaults:
test_the_letterboxed_clip_of_the_gpu_tests_gives_its_rectangle asserts it here."""
import configparser
import os
import re
import sys
from fractions import Fraction as Fr

import numpy as np
import pytest

from ssm_amd import video as V

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from video_active_clips import FH, FW, RECT, letterboxed  # noqa: E402

LAYOUTS = (V.CENTRED, V.COSITED, V.C422, V.C444)
ALIGN = {V.CENTRED: (2, 2), V.COSITED: (2, 2), V.C422: (1, 2), V.C444: (1, 1)}          # (rows, columns)


def frame(h, w, layout, bits, fill=0):
    x = np.zeros(V.frame_bytes(h, w, layout, bits), np.uint8)
    for p in V.split_planes(x.reshape(1, -1), h, w, layout, bits):
        p[...] = fill
    return x


def luma(x, h, w, layout, bits):
    return V.split_planes(x.reshape(1, -1), h, w, layout, bits)[0][0]


# ---- counts ------------------------------------------------------------------------------------------------------------------------------
def test_counts_on_hand_made_planes():
    x = frame(4, 6, V.C444, 8)
    y = luma(x, 4, 6, V.C444, 8)
    y[1, 2:5] = (25, 24, 200)          # 24 is not above the default limit
    y[3, 0] = 255
    rows, cols = V.active_counts_host(x, 4, 6, 8)
    assert rows.dtype == np.uint32 and cols.dtype == np.uint32
    assert rows.tolist() == [0, 2, 0, 1] and cols.tolist() == [1, 0, 1, 0, 1, 0]
    rows, cols = V.active_counts_host(x, 4, 6, 8, 0)          # limit 0: every sample above 0
    assert rows.tolist() == [0, 3, 0, 1] and cols.tolist() == [1, 0, 1, 1, 1, 0]
    assert V.active_counts_host(x, 4, 6, 8, 255)[0].tolist() == [0, 0, 0, 0]          # nothing is above the peak


def test_counts_do_not_look_at_chroma_and_words_count_whole():
    x = frame(4, 6, V.CENTRED, 8)
    u = V.split_planes(x.reshape(1, -1), 4, 6, V.CENTRED, 8)[1]
    u[...] = 255
    assert V.active_counts_host(x, 4, 6, 8)[0].sum() == 0
    x = frame(3, 5, V.C422, 10)
    y = luma(x, 3, 5, V.C422, 10)
    y[2, 4], y[0, 0] = 97, 96          # the default limit at 10 bits is 24 * 4 = 96
    rows, cols = V.active_counts_host(np.stack([x, x]), 3, 5, 10)
    assert rows.shape == (2, 3) and cols.shape == (2, 5) and rows[1].tolist() == [0, 0, 1] and cols[0].tolist() == [0, 0, 0, 0, 1]
    y[1, 1] = 0xff00          # a word is compared whole, all 16 bits
    assert V.active_counts_host(x, 3, 5, 16, 0xfeff)[0].tolist() == [0, 1, 0]
    assert V.active_limit(8) == 24 and V.active_limit(10) == 96 and V.active_limit(16) == 24 * 256 and V.active_limit(10, 7) == 7


# ---- the decision --------------------------------------------------------------------------------------------------------------------------
def boxed(h, w, layout, bits, y0, y1, x0, x1, value=None):
    """A frame whose luma is bright in rows y0 .. y1 - 1 and columns x0 .. x1 - 1 and black elsewhere."""
    x = frame(h, w, layout, bits)
    luma(x, h, w, layout, bits)[y0:y1, x0:x1] = (200 << (bits - 8)) if value is None else value
    return x


def test_union_over_frames_and_the_probe():
    h, w = 64, 96
    a, b, c = boxed(h, w, V.C444, 8, 10, 50, 4, 90), boxed(h, w, V.C444, 8, 8, 40, 6, 92), boxed(h, w, V.C444, 8, 0, 64, 0, 96)
    rect, area = V.active_area_host(np.stack([a, b]), h, w, V.C444)
    assert rect == (88, 42, 4, 8) and area.fed == 2 and "88:42:4:8" in area.note
    assert V.active_area_host(np.stack([a, b, c]), h, w, V.C444, probe=2)[0] == rect, "frames behind the probe are not looked at"
    assert V.active_area_host(np.stack([a, b, c]), h, w, V.C444, probe=3)[0] is None
    assert V.active_area_host(np.stack([a]), h, w, V.C444, probe=48)[0] == (86, 40, 4, 10), "a clip shorter than the probe"


@pytest.mark.parametrize("layout", LAYOUTS)
def test_alignment_goes_outward_on_every_layout(layout):
    ay, ax = ALIGN[layout]
    assert V.active_align(layout) == (ay, ax)
    h, w = 81, 101          # odd H and W
    x = boxed(h, w, layout, 8, 11, 64, 13, 88)
    want = (88 + (88 % ax) - (13 - 13 % ax), 64 + (64 % ay) - (11 - 11 % ay), 13 - 13 % ax, 11 - 11 % ay)
    assert V.active_area_host(x[None], h, w, layout)[0] == want
    rw, rh, x0, y0 = want
    assert x0 % ax == 0 and y0 % ay == 0 and (x0 + rw) % ax == 0 and (y0 + rh) % ay == 0
    # a far edge on the frame's own odd edge stays there
    x = boxed(h, w, layout, 8, 11, 81, 13, 101)
    assert V.active_area_host(x[None], h, w, layout)[0] == (101 - (13 - 13 % ax), 81 - (11 - 11 % ay), 13 - 13 % ax, 11 - 11 % ay)
    # and one row and column short of it rounds up to it or stays
    x = boxed(h, w, layout, 8, 11, 80, 13, 100)
    rw, rh, x0, y0 = V.active_area_host(x[None], h, w, layout)[0]
    assert (y0 + rh, x0 + rw) == (80 if ay == 1 or 80 % ay == 0 else 81, 100 if 100 % ax == 0 else 101)


def test_whole_frame_fallbacks():
    h, w = 64, 96
    rect, area = V.active_area_host(boxed(h, w, V.CENTRED, 8, 0, 64, 0, 96)[None], h, w, V.CENTRED)
    assert rect is None and area.note == "the active area is the whole frame"
    rect, area = V.active_area_host(boxed(h, w, V.CENTRED, 8, 1, 64, 1, 96)[None], h, w, V.CENTRED)
    assert rect is None and "whole frame" in area.note, "aligned outward it is the whole frame"
    rect, area = V.active_area_host(np.stack([frame(h, w, V.CENTRED, 8, 16)] * 3), h, w, V.CENTRED)
    assert rect is None and area.note == "no active row or column in the 3 probed frames"
    rect, area = V.active_area_host(boxed(h, w, V.CENTRED, 8, 10, 40, 20, 50)[None], h, w, V.CENTRED)
    assert rect is None and "30:30:20:10 is under 32 samples" in area.note
    assert V.active_area_host(boxed(h, w, V.CENTRED, 8, 10, 42, 20, 52)[None], h, w, V.CENTRED)[0] == (32, 32, 20, 10)
    assert V.active_area_host(boxed(h, w, V.CENTRED, 8, 10, 42, 20, 51)[None], h, w, V.CENTRED)[0] == (32, 32, 20, 10), "31 columns align to 32"
    assert V.active_area_host(boxed(h, w, V.C444, 8, 10, 42, 20, 51)[None], h, w, V.C444)[0] is None, "and stay 31 in 4:4:4"


def test_frac_is_a_strict_inequality():
    h, w = 64, 128          # 1/64 of a row is exactly 2 samples, of a column exactly 1
    x = frame(h, w, V.C444, 8)
    y = luma(x, h, w, V.C444, 8)
    y[10:50, 20:22] = 200          # rows 10 .. 49 hold 2 bright samples: not above 2;  columns 20, 21 hold 40: above 1
    area = V.ActiveArea(h, w, V.C444)
    rows, cols = V.active_counts_host(x, h, w, 8)
    ar, ac = area.lines(rows, cols)
    assert not ar.any() and np.flatnonzero(ac).tolist() == [20, 21]
    assert V.active_area_host(x[None], h, w, V.C444)[0] is None
    y[10:50, 22] = 200             # 3 samples: above
    ar, ac = area.lines(*V.active_counts_host(x, h, w, 8))
    assert np.flatnonzero(ar).tolist() == list(range(10, 50)) and np.flatnonzero(ac).tolist() == [20, 21, 22]
    y[:] = 0
    y[7, :] = 200
    y[7, 5] = 0                    # a column with one bright sample holds exactly 1/64 of 64: not active; the row is
    ar, ac = area.lines(*V.active_counts_host(x, h, w, 8))
    assert np.flatnonzero(ar).tolist() == [7] and not ac.any()
    y[8, :] = 200
    ar, ac = area.lines(*V.active_counts_host(x, h, w, 8))
    assert ac.sum() == 127 and not ac[5], "two samples are above 1; column 5 holds one, exactly 1/64"
    # another FRAC: 1/2 of 128 columns is 64
    half = V.ActiveArea(h, w, V.C444, Fr(1, 2))
    y[:] = 0
    y[3, :64], y[4, :65] = 200, 200
    assert np.flatnonzero(half.lines(*V.active_counts_host(x, h, w, 8))[0]).tolist() == [4]


def test_outside_counts_active_lines_beyond_the_rectangle():
    h, w = 64, 96
    area = V.ActiveArea(h, w, V.CENTRED)
    x = boxed(h, w, V.CENTRED, 8, 10, 50, 4, 90)
    assert area.outside(*V.active_counts_host(x, h, w, 8), (86, 40, 4, 10)) == (0, 0)
    assert area.outside(*V.active_counts_host(x, h, w, 8), (80, 36, 6, 12)) == (4, 6)


def test_the_letterboxed_clip_of_the_gpu_tests_gives_its_rectangle():
    for tag in ("420jpeg", "422p10"):
        layout, bits = V.EXTENDED_TAGS[tag]
        clip, picture = letterboxed(tag)
        assert V.active_area_host(clip, FH, FW, layout, bits)[0] == RECT
        assert V.active_area_host(clip, FH, FW, layout, bits, probe=2)[0] == RECT
        assert np.array_equal(V.cut_window_host(clip, FH, FW, layout, bits, RECT), picture)
        bars = clip.copy()
        V.paste_window_host(np.zeros_like(picture), bars, FH, FW, layout, bits, RECT, out=bars)
        assert all(len(np.unique(bars[i])) > 3 for i in range(len(bars))), "the bars carry a subtitle"
        assert len({bars[i].tobytes() for i in range(len(bars))}) == len(bars), "which changes every frame"


# ---- the window copies ---------------------------------------------------------------------------------------------------------------------
def rects_of(h, w, layout):
    """A window at each corner, the whole frame and the smallest aligned window (inside, and on the far edges) of an h x w frame."""
    ay, ax = ALIGN[layout]
    my, mx = (h // 2) - (h // 2) % ay, (w // 2) - (w // 2) % ax
    return [(mx, my, 0, 0), (w - mx, my, mx, 0), (mx, h - my, 0, my), (w - mx, h - my, mx, my), (w, h, 0, 0), (ax, ay, mx, my),
            (w - (w - 1) // ax * ax, h - (h - 1) // ay * ay, (w - 1) // ax * ax, (h - 1) // ay * ay)]


@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_cut_then_paste_is_the_identity(layout, bits):
    rng = np.random.RandomState(3)
    for h, w in ((17, 23), (16, 24), (6, 9)):
        fb = V.frame_bytes(h, w, layout, bits)
        f, g = (rng.randint(0, 256, (2, fb)).astype(np.uint8) for _ in range(2))
        for rect in rects_of(h, w, layout):
            win = V.cut_window_host(f, h, w, layout, bits, rect)
            assert win.shape == (2, V.frame_bytes(rect[1], rect[0], layout, bits)), "a genuine h' x w' frame of the layout"
            assert np.array_equal(V.paste_window_host(win, f, h, w, layout, bits, rect), f)
            mixed = V.paste_window_host(win, g, h, w, layout, bits, rect)
            assert np.array_equal(V.cut_window_host(mixed, h, w, layout, bits, rect), win)
            back = V.paste_window_host(V.cut_window_host(g, h, w, layout, bits, rect), mixed, h, w, layout, bits, rect)
            assert np.array_equal(back, g), "outside the rectangle the bytes are bars_from's, in all three planes"
            one = V.cut_window_host(f[0], h, w, layout, bits, rect)
            assert one.shape == win.shape[1:] and np.array_equal(one, win[0])


def test_chroma_bounds_for_odd_sizes():
    h, w = 7, 9
    x = np.zeros((1, V.frame_bytes(h, w, V.CENTRED, 8)), np.uint8)
    y, u, v = V.split_planes(x, h, w, V.CENTRED, 8)
    y[0] = np.arange(h * w).reshape(h, w)
    u[0] = 100 + np.arange(4 * 5).reshape(4, 5)
    v[0] = 200 + np.arange(4 * 5).reshape(4, 5)
    win = V.cut_window_host(x, h, w, V.CENTRED, 8, (5, 3, 4, 4))[0:1]          # rows 4 .. 6, columns 4 .. 8: to both far edges
    wy, wu, wv = V.split_planes(win, 3, 5, V.CENTRED, 8)
    assert np.array_equal(wy[0], y[0, 4:7, 4:9])
    assert wu.shape == (1, 2, 3) and np.array_equal(wu[0], u[0, 2:4, 2:5]) and np.array_equal(wv[0], v[0, 2:4, 2:5]), \
        "chroma from y / 2 to ceil((y + h') / 2)"
    x2 = np.zeros((1, V.frame_bytes(h, w, V.C422, 8)), np.uint8)
    y2, u2, _ = V.split_planes(x2, h, w, V.C422, 8)
    u2[0] = np.arange(7 * 5).reshape(7, 5)
    wu = V.split_planes(V.cut_window_host(x2, h, w, V.C422, 8, (3, 2, 6, 1)), 2, 3, V.C422, 8)[1]
    assert np.array_equal(wu[0], u2[0, 1:3, 3:5]), "4:2:2: every row, columns x / 2 to ceil((x + w') / 2)"


# ---- the option ----------------------------------------------------------------------------------------------------------------------------
def test_parse_active_takes_every_form():
    assert V.parse_active(None) is None
    assert V.parse_active("auto") == ("auto", None, Fr(1, 64))
    assert V.parse_active("auto:30") == ("auto", 30, Fr(1, 64))
    assert V.parse_active("auto:30:1/32") == ("auto", 30, Fr(1, 32))
    assert V.parse_active("auto:96:0.25") == ("auto", 96, Fr(1, 4))
    assert V.parse_active("auto::1/8") == ("auto", None, Fr(1, 8))
    assert V.parse_active("1920:800:0:140") == (1920, 800, 0, 140)
    assert V.parse_active("crop=1920:800:0:140") == (1920, 800, 0, 140), "cropdetect's line can be pasted"
    assert V.parse_active((96, 64, 8, 16)) == (96, 64, 8, 16)
    assert V.parse_active(("auto", None, Fr(1, 64))) == ("auto", None, Fr(1, 64))
    for bad in ("", "auto:x", "auto:1:2:3", "auto:24:1", "auto:-1", "auto:70000", "1:2:3", "1:2:3:4:5", "a:b:c:d", "0:8:0:0", "8:8:-2:0",
                (1, 2, 3), (1.5, 2, 0, 0), True, 7):
        with pytest.raises(ValueError, match="auto, auto:LIM, auto:LIM:FRAC or W:H:X:Y"):
            V.parse_active(bad)
    assert V.parse_active_probe(48) == 48 and V.parse_active_probe("3") == 3
    for bad in (0, -1, "x", 1.5, True):
        with pytest.raises(ValueError, match="active_probe"):
            V.parse_active_probe(bad)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_misaligned_or_outside_rectangle_is_refused_by_a_message_that_names_the_alignment(layout):
    ay, ax = ALIGN[layout]
    h, w = 65, 97
    assert V.check_active((96, 64, 0, 0), h, w, layout) == (96, 64, 0, 0)
    assert V.check_active((97, 65, 0, 0), h, w, layout) == (97, 65, 0, 0), "the frame's own odd edges are fine"
    named = "%d columns and %d rows" % (ax, ay)
    for rect in ((96, 64, 2, 2), (98, 10, 0, 0), (10, 66, 0, 0), (1, 1, 97, 0)):
        with pytest.raises(ValueError, match=r"lies outside the 97x65 frame.*%s" % named):
            V.check_active(rect, h, w, layout)
    wrong = [r for r, a in (((10, 10, 1, 0), ax), ((11, 10, 0, 0), ax), ((10, 10, 0, 1), ay), ((10, 11, 0, 0), ay)) if a == 2]
    for rect in wrong:
        with pytest.raises(ValueError, match=r"is not aligned to %s" % named):
            V.check_active(rect, h, w, layout)
    if layout == V.C444:
        assert V.check_active((11, 11, 1, 1), h, w, layout) == (11, 11, 1, 1)


class _Model:
    recurrent = False
    precision = None


class _Recurrent(_Model):
    recurrent = True


def _cfg():
    cfg = configparser.RawConfigParser()
    cfg.read_dict({"TRAIN": {"N_FRAMES": "2"}})
    return cfg


def test_interpolator_takes_the_option_and_refuses_what_does_not_go_with_it():
    vi = V.VideoInterpolator(_Model(), _cfg())
    assert vi.active_option is None and vi.active is None and vi.active_excess == [] and vi.active_probe == 48
    vi = V.VideoInterpolator(_Model(), _cfg(), upsample_rate=2, active="auto", active_probe=5)
    assert vi.active_option == ("auto", None, Fr(1, 64)) and vi.active_probe == 5 and vi.active is None
    vi = V.VideoInterpolator(_Model(), _cfg(), target_rate=(60, 1), scene_cut="1/10", flow_scale=2, active=(96, 64, 8, 16))
    assert vi.active_option == (96, 64, 8, 16)
    assert V.VideoInterpolator(_Model(), _cfg(), speed="1/2", active="96:64:8:16").active_option == (96, 64, 8, 16)
    for name, kw, model in (("shutter", dict(shutter="1/2", speed=1), _Model), ("deinterlace", dict(deinterlace="tff"), _Model),
                            ("dedup", dict(dedup=True), _Model), ("a recurrent model", {}, _Recurrent)):
        with pytest.raises(ValueError, match="active together with %s is not available.*chain two runs" % name):
            V.VideoInterpolator(model(), _cfg(), active="auto", **kw)
    with pytest.raises(ValueError, match="W:H:X:Y"):
        V.VideoInterpolator(_Model(), _cfg(), active="1:2:3")
    with pytest.raises(ValueError, match="active_probe"):
        V.VideoInterpolator(_Model(), _cfg(), active="auto", active_probe=0)


def test_clip_with_a_window_has_two_sizes_and_the_windows_canvas():
    plain = V.Clip(96, 112, V.CENTRED, V.BT601, V.LIMITED)
    assert plain.fb == plain.fb_in == plain.fb_out == V.frame_bytes(96, 112, V.CENTRED) and plain.window is None
    assert (plain.h, plain.w, plain.hp, plain.wp) == (96, 112, 96, 128)
    clip = V.Clip(96, 112, V.CENTRED, V.BT601, V.LIMITED, window=(96, 64, 8, 16))
    assert clip.frame == (96, 112) and (clip.h, clip.w, clip.hp, clip.wp, clip.at) == (64, 96, 64, 96, (0, 0))
    assert clip.fb == clip.fb_in == V.frame_bytes(96, 112, V.CENTRED) and clip.fb_out == V.frame_bytes(64, 96, V.CENTRED)
    with pytest.raises(ValueError, match="not aligned to 2 columns and 2 rows"):
        V.Clip(96, 112, V.CENTRED, V.BT601, V.LIMITED, window=(96, 64, 8, 15))


BASE = ["-c", "x.ini", "--expt", "e", "--log", "l", "--input", "-", "--output", "-"]


def test_cli_flags():
    import interpolate_video as cli
    a = cli.getargs(BASE)
    assert a.active is None and a.active_probe == 48 and a.upsample_rate == 8, "without the flag the tool is as it was"
    a = cli.getargs(BASE + ["--active", "auto"])
    assert a.active == ("auto", None, Fr(1, 64)) and a.upsample_rate == 8
    a = cli.getargs(BASE + ["--active", "auto:30:1/32", "--active_probe", "12", "--fps", "60", "--scene_cut", "0.1", "--detelecine", "--tile",
                            "64x64", "--matrix", "bt709", "--range", "full"])
    assert a.active == ("auto", 30, Fr(1, 32)) and a.active_probe == 12
    a = cli.getargs(BASE + ["--active", "1920:800:0:140", "--upsample_rate", "4", "--slowmo", "--flow_scale", "2"])
    assert a.active == (1920, 800, 0, 140)
    assert cli.getargs(BASE + ["--active", "crop=1920:800:0:140", "--speed", "1/2"]).active == (1920, 800, 0, 140)


@pytest.mark.parametrize("flags,named", [(["--speed", "1", "--shutter", "180"], "--shutter"), (["--deinterlace", "auto"], "--deinterlace"),
                                         (["--dedup"], "--dedup")])
def test_cli_refuses_by_name_and_points_to_two_runs(capsys, flags, named):
    import interpolate_video as cli
    with pytest.raises(SystemExit) as e:
        cli.getargs(BASE + ["--active", "auto"] + flags)
    assert e.value.code == 2
    assert re.search(r"--active does not go together with %s: .* chain two runs" % named, capsys.readouterr().err)


def test_cli_refuses_bad_values(capsys):
    import interpolate_video as cli
    for flags, text in ((["--active", "1:2:3"], "W:H:X:Y"), (["--active", "auto", "--active_probe", "0"], "active_probe")):
        with pytest.raises(SystemExit):
            cli.getargs(BASE + flags)
        assert text in capsys.readouterr().err


# ---- the entry points: every refusal, nothing queued ---------------------------------------------------------------------------------------------
P, Q, R = 0x10000, 0x20000, 0x30000          # addresses that are never followed: every call below is refused before anything is queued


@pytest.mark.parametrize("args,message", [
    ((None, 64, 1, 8, 8, 1, 24, Q, R), "luma_counts: null pointer"),
    ((P, 64, 1, 8, 8, 1, 24, None, R), "luma_counts: null pointer"),
    ((P, 64, 1, 8, 8, 1, 24, Q, None), "luma_counts: null pointer"),
    ((P, 64, 0, 8, 8, 1, 24, Q, R), "luma_counts: N=0 outside 1..65535"),
    ((P, 64, 65536, 8, 8, 1, 24, Q, R), "luma_counts: N=65536 outside 1..65535"),
    ((P, 64, 1, 0, 8, 1, 24, Q, R), "luma_counts: bad plane size 0x8"),
    ((P, 64, 1, 8, -1, 1, 24, Q, R), "luma_counts: bad plane size 8x-1"),
    ((P, 64, 1, 8, 8, 0, 24, Q, R), "luma_counts: sample_bytes 0 not in {1, 2}"),
    ((P, 64, 1, 8, 8, 3, 24, Q, R), "luma_counts: sample_bytes 3 not in {1, 2}"),
    ((P, 63, 2, 8, 8, 1, 24, Q, R), "luma_counts: stride 63 shorter than the plane's 64 bytes"),
    ((P, -127, 2, 8, 8, 2, 24, Q, R), "luma_counts: stride -127 shorter than the plane's 128 bytes"),
    ((P + 1, 128, 2, 8, 8, 2, 24, Q, R), "luma_counts: a plane of 2-byte samples is not 2-byte aligned"),
    ((P, 129, 2, 8, 8, 2, 24, Q, R), "luma_counts: stride 129 of 2-byte samples must be even"),
    ((P, 64, 1, 8, 8, 1, -1, Q, R), "luma_counts: limit=-1 outside 0..65535"),
    ((P, 64, 1, 8, 8, 1, 65536, Q, R), "luma_counts: limit=65536 outside 0..65535"),
    ((P, 64, 1, 8, 8, 1, 24, Q + 2, R), "luma_counts: rows or cols is not 4-byte aligned"),
    ((P, 64, 1, 8, 8, 1, 24, Q, R + 1), "luma_counts: rows or cols is not 4-byte aligned"),
    ((P, 0, 1, 1 << 22, 8, 1, 24, Q, R), "luma_counts: a plane of 4194304 rows is more than the grid takes"),
])
def test_luma_counts_refusals(args, message):
    from ssm_amd import hipbind as hb
    lib = hb.load()
    assert lib.ssm_luma_counts_fwd(*args, None) == -1
    assert lib.ssm_last_error_string().decode() == message


FB, WB = 16 * 16 * 3, 8 * 8 * 3          # a 16 x 16 frame and an 8 x 8 window in 4:4:4 (layout 2)


@pytest.mark.parametrize("args,message", [
    ((None, FB, Q, WB, 1, 16, 16, 0, 0, 8, 8, 2, 1), "window_cut: null pointer"),
    ((P, FB, None, WB, 1, 16, 16, 0, 0, 8, 8, 2, 1), "window_cut: null pointer"),
    ((P, FB, Q, WB, 0, 16, 16, 0, 0, 8, 8, 2, 1), "window_cut: N=0 outside 1..65535"),
    ((P, FB, Q, WB, 1, 0, 16, 0, 0, 8, 8, 2, 1), "window_cut: bad frame size 0x16"),
    ((P, FB, Q, WB, 1, 16, 16, 0, 0, 8, 8, 4, 1), "window_cut: layout 4 not in {0, 1, 2, 3}"),
    ((P, FB, Q, WB, 1, 16, 16, 0, 0, 8, 8, 2, 3), "window_cut: sample_bytes 3 not in {1, 2}"),
    ((P, FB, Q, WB, 1, 16, 16, 0, 0, 0, 8, 2, 1), "window_cut: the window 0x8 at (0,0) (h x w at y, x) lies outside the 16x16 frame"),
    ((P, FB, Q, WB, 1, 16, 16, 9, 0, 8, 8, 2, 1), "window_cut: the window 8x8 at (9,0) (h x w at y, x) lies outside the 16x16 frame"),
    ((P, FB, Q, WB, 1, 16, 16, 0, -1, 8, 8, 2, 1), "window_cut: the window 8x8 at (0,-1) (h x w at y, x) lies outside the 16x16 frame"),
    ((P, FB, Q, WB, 1, 16, 16, 0, 12, 8, 8, 2, 1), "window_cut: the window 8x8 at (0,12) (h x w at y, x) lies outside the 16x16 frame"),
    ((P, FB, Q, WB, 1, 16, 16, 1, 0, 8, 8, 0, 1), "window_cut: the window 8x8 at (1,0) is not aligned to (2,2) rows and columns, as layout 0 asks: "
                                                  "its origin a multiple, its far edges a multiple or the frame's own"),
    ((P, FB, Q, WB, 1, 16, 16, 0, 0, 7, 8, 1, 1), "window_cut: the window 7x8 at (0,0) is not aligned to (2,2) rows and columns, as layout 1 asks: "
                                                  "its origin a multiple, its far edges a multiple or the frame's own"),
    ((P, FB, Q, WB, 1, 16, 16, 1, 1, 8, 8, 3, 1), "window_cut: the window 8x8 at (1,1) is not aligned to (1,2) rows and columns, as layout 3 asks: "
                                                  "its origin a multiple, its far edges a multiple or the frame's own"),
    ((P + 1, 2 * FB, Q, 2 * WB, 2, 16, 16, 0, 0, 8, 8, 2, 2), "window_cut: a payload of 2-byte samples (frames or windows) is not 2-byte aligned"),
    ((P, 2 * FB + 1, Q, 2 * WB, 2, 16, 16, 0, 0, 8, 8, 2, 2), "window_cut: strides 1537 (frames), 384 (windows) of 2-byte samples must be even"),
    ((P, FB - 1, Q, WB, 2, 16, 16, 0, 0, 8, 8, 2, 1), "window_cut: stride 767 (frames) shorter than the frame's 768 bytes"),
    ((P, FB, Q, WB - 1, 2, 16, 16, 0, 0, 8, 8, 2, 1), "window_cut: stride 191 (windows) shorter than the window's 192 bytes"),
    ((P, FB, P + 100, WB, 2, 16, 16, 0, 0, 8, 8, 2, 1), "window_cut: windows overlaps frames"),
])
def test_window_cut_refusals(args, message):
    from ssm_amd import hipbind as hb
    lib = hb.load()
    assert lib.ssm_window_cut_fwd(*args, None) == -1
    assert lib.ssm_last_error_string().decode() == message


def test_window_cut_takes_the_frames_own_odd_edges():
    """Refusals come before anything is queued; an aligned call on a null stream would launch, so the legal cases are told apart by their message:
    a window to the odd far edges of a 17 x 23 frame passes the alignment check and is refused only later, for the overlap."""
    from ssm_amd import hipbind as hb
    lib = hb.load()
    assert lib.ssm_window_cut_fwd(P, 0, P, 0, 1, 17, 23, 10, 14, 7, 9, 0, 1, None) == -1
    assert lib.ssm_last_error_string().decode() == "window_cut: windows overlaps frames"
