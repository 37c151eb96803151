"""Repeated frames without a GPU: the definition in numpy (block_counts, block_sad_host, Repeats, dedup_host), the gap
timeline through PassPlanner, parse_dedup and the option refusals of VideoInterpolator and the command line, and the refusals of
ssm_block_sad_fwd through the library as tests/test_cabi_cpu.py loads it.

The synthetic moving clip of tests/video_clips.py, at the size the streamed GPU tests use (tests/test_hip_video_dedup.py), must hold no
repeat under the default thresholds: test_moving_clip_has_no_repeat_under_the_defaults asserts it, so the streamed tests run with
dedup=True where they mean the defaults."""
import os
import re
import sys
from fractions import Fraction as Fr

import numpy as np
import pytest

from ssm_amd import video as V

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from video_clips import clip_payloads  # noqa: E402

H, W = 64, 96          # the frame of the streamed GPU tests


def frames_of(h, w, layout, bits, n=2, fill=0):
    x = np.full((n, V.frame_bytes(h, w, layout, bits)), fill, np.uint8)
    return x


def planes(x, h, w, layout, bits):
    return V.split_planes(x, h, w, layout, bits)


# ---- blocks ----------------------------------------------------------------------------------------------------------------------------
def test_block_counts():
    assert V.block_counts(8, 8, V.CENTRED) == (1, 0, 0), "a 4:2:0 frame of 8 x 8 has one Y block and no chroma block"
    assert V.block_counts(7, 64, V.C444) == (0, 0, 0)
    assert V.block_counts(17, 23, V.CENTRED) == (4, 1, 1)          # chroma 9 x 12
    assert V.block_counts(16, 24, V.C422) == (6, 2, 2)             # chroma 16 x 12
    assert V.block_counts(64, 96, V.C444) == (96, 96, 96)
    assert V.block_counts(720, 1280, V.CENTRED) == (14400, 3600, 3600)


def test_trailing_columns_and_rows_count_nothing():
    h, w = 19, 29          # Y: 2 x 3 blocks, rows 16.., columns 24.. belong to none; 4:4:4 so that U and V are the same
    a = frames_of(h, w, V.C444, 8)
    b = a.copy()
    for p in planes(b, h, w, V.C444, 8):
        p[:, 16:, :] = 255
        p[:, :, 24:] = 255
    assert not np.array_equal(a, b)
    assert V.block_sad_host(a, b, h, w, V.C444, lo=0).tolist() == [[[0, 0]] * 3] * 2


def test_one_sample_in_one_block_and_the_lo_threshold():
    h, w = 16, 24
    a = frames_of(h, w, V.C444, 8, 1)
    b = a.copy()
    planes(b, h, w, V.C444, 8)[1][0, 9, 17] = 37          # U, block (2, 1)
    assert V.block_sad_host(a, b, h, w, V.C444, lo=0).tolist() == [[[0, 0], [37, 1], [0, 0]]]
    assert V.block_sad_host(a, b, h, w, V.C444, lo=37).tolist() == [[[0, 0], [37, 0], [0, 0]]], "d == lo is not over"
    assert V.block_sad_host(a, b, h, w, V.C444, lo=36).tolist() == [[[0, 0], [37, 1], [0, 0]]], "d == lo + 1 is over"
    planes(b, h, w, V.C444, 8)[1][0, 15, 23] = 3          # the same block: sums add, the count stays
    planes(b, h, w, V.C444, 8)[1][0, 0, 0] = 5            # another block
    assert V.block_sad_host(a, b, h, w, V.C444, lo=4).tolist() == [[[0, 0], [40, 2], [0, 0]]]
    assert V.block_sad_host(b, a, h, w, V.C444, lo=4).tolist() == [[[0, 0], [40, 2], [0, 0]]], "|a - b| is symmetric"


def test_8x8_frame_in_420_has_one_luma_block_and_no_chroma_block():
    a = frames_of(8, 8, V.CENTRED, 8, 1)
    b = frames_of(8, 8, V.CENTRED, 8, 1, fill=255)
    assert V.block_sad_host(a, b, 8, 8, V.CENTRED).tolist() == [[[64 * 255, 1], [0, 0], [0, 0]]]


def test_words_count_all_16_bits_and_one_row_goes_against_n():
    h, w = 8, 16
    a = frames_of(h, w, V.C422, 16, 1)
    b = frames_of(h, w, V.C422, 16, 3, fill=255)
    planes(b[2:], h, w, V.C422, 16)[0][0, :, 8:] = 0
    got = V.block_sad_host(a, b, h, w, V.C422, 16, lo=64 * 65535 - 1)
    assert got.dtype == np.uint64 and got.shape == (3, 3, 2)
    assert got[0].tolist() == [[64 * 65535, 2], [64 * 65535, 1], [64 * 65535, 1]] and got[2, 0].tolist() == [64 * 65535, 1]
    assert 64 * 65535 < V.BLOCK_SAD_MAX
    assert V.block_sad_host(a, b, h, w, V.C422, 16)[0, 0].tolist() == [64 * 65535, 2], "the default lo is 320 << 8"


# ---- the decision ------------------------------------------------------------------------------------------------------------------------
REP, NEW = (0, 0) * 3, (1000, 1) * 3          # the words of an exact repeat, and of a frame that is none under (0, 0, 0)


def decide(flags, dedup_max=2, blocks=(96, 24, 24), th=(0, 0, 0)):
    """The actions and log of a clip whose frames 1 .. are repeats where `flags` says so."""
    rep = V.Repeats(*th, blocks, dedup_max)
    out = []
    for f in flags:
        out += rep.feed(REP if f else NEW)
    return out + rep.end(), rep.log


def test_runs_of_length_d_and_d_plus_one():
    # frames: 0 | 1 2 repeats | 3 new | 4 5 6 repeats (a still) | 7 new
    acts, log = decide([1, 1, 0, 1, 1, 1, 0])
    assert acts == [(0, None), (1, (0, 3, Fr(1, 3))), (2, (0, 3, Fr(2, 3))), (3, None), (4, None), (5, None), (6, None), (7, None)]
    assert log == [(1, 2, True, 0, 0), (4, 3, False, 0, 0)]
    acts, log = decide([1, 1, 0, 1, 1, 1, 0], dedup_max=3)
    assert acts[4:7] == [(4, (3, 7, Fr(1, 4))), (5, (3, 7, Fr(1, 2))), (6, (3, 7, Fr(3, 4)))] and log[1] == (4, 3, True, 0, 0)
    acts, log = decide([0, 1, 0, 0], dedup_max=1)
    assert acts == [(0, None), (1, None), (2, (1, 3, Fr(1, 2))), (3, None), (4, None)] and log == [(2, 1, True, 0, 0)]


def test_a_run_at_the_end_and_a_run_from_frame_one():
    acts, log = decide([1, 0, 0, 1, 1])
    assert acts == [(0, None), (1, (0, 2, Fr(1, 2))), (2, None), (3, None), (4, None), (5, None)]
    assert log == [(1, 1, True, 0, 0), (4, 2, False, 0, 0)], "a run at the clip's end has no right neighbour"
    assert decide([]) == ([(0, None)], [])
    assert decide([1]) == ([(0, None), (1, None)], [(1, 1, False, 0, 0)])


def test_frames_close_as_soon_as_they_can():
    rep = V.Repeats(0, 0, 0, (1, 0, 0))
    assert rep.feed(REP) == [(0, None)] and rep.feed(REP) == []          # two repeats wait
    assert rep.feed(REP) == [(1, None), (2, None), (3, None)]            # the third makes it a still
    assert rep.feed(REP) == [(4, None)] and rep.log == []                # and the still goes on, one frame at a time
    assert rep.feed(NEW) == [(5, None)] and rep.log == [(1, 4, False, 0, 0)]
    assert rep.feed(REP) == [] and rep.feed(NEW) == [(6, (5, 7, Fr(1, 2))), (7, None)] and rep.end() == []


def test_thresholds_floor_of_a_fraction_and_planes_without_blocks():
    # 10 blocks at frac = 33/100: floor(3.3) = 3 blocks may be over lo
    rep = V.Repeats(768, 320, Fr(33, 100), (10, 10, 10))
    assert rep.allowed == (3, 3, 3)
    assert rep.is_repeat((768, 3, 768, 3, 768, 3)) and not rep.is_repeat((769, 0, 0, 0, 0, 0)) and not rep.is_repeat((0, 0, 0, 4, 0, 0))
    assert V.Repeats(0, 0, Fr(1, 3), (3, 2, 2)).allowed == (1, 0, 0) and V.Repeats(0, 0, Fr(299, 300), (300, 0, 0)).allowed == (299, 0, 0)
    # a plane without blocks is not consulted, whatever its words say
    lone = V.Repeats(0, 0, 0, (1, 0, 0))
    assert lone.is_repeat((0, 0, 99999, 7, 99999, 7)) and not lone.is_repeat((1, 0, 0, 0, 0, 0))
    assert V.Repeats(0, 0, 0, (0, 0, 0)).is_repeat((5, 5, 5, 5, 5, 5)), "a frame without any block repeats: nothing says otherwise"


def test_log_keeps_the_worst_of_a_run():
    rep = V.Repeats(768, 320, Fr(1, 2), (8, 2, 2))
    out = rep.feed((700, 4, 10, 0, 0, 0)) + rep.feed((5, 0, 20, 1, 768, 0)) + rep.feed((769, 0, 0, 0, 0, 0))
    assert [a is not None for _, a in out] == [False, True, True, False]
    assert rep.log == [(1, 2, True, 768, 4)]


def test_dedup_host_on_a_clip_with_exact_and_near_repeats():
    h, w = 16, 24
    rng = np.random.RandomState(3)
    base = rng.randint(0, 256, size=(4, V.frame_bytes(h, w, V.CENTRED))).astype(np.uint8)
    near = base[1].copy()
    near[::7] = np.clip(near[::7].astype(int) + 1, 0, 255)          # under the defaults a repeat, under (0, 0, 0) none
    clip = np.stack([base[0], base[0], base[1], near, near, base[2], base[3], base[3]])
    acts, rep = V.dedup_host(clip, h, w, V.CENTRED)
    assert [a for _, a in acts] == [None, (0, 2, Fr(1, 2)), None, (2, 5, Fr(1, 3)), (2, 5, Fr(2, 3)), None, None, None]
    assert [r[:3] for r in rep.log] == [(1, 1, True), (3, 2, True), (7, 1, False)] and rep.log[1][3] > 0
    acts, rep = V.dedup_host(clip, h, w, V.CENTRED, dedup=(0, 0, 0))
    assert [a for _, a in acts] == [None, (0, 2, Fr(1, 2)), None, None, (3, 5, Fr(1, 2)), None, None, None]


def test_moving_clip_has_no_repeat_under_the_defaults():
    """What lets the streamed GPU tests use dedup=True on clips built from this one: no two consecutive frames of it pass for repeats."""
    for siting in (V.CENTRED, V.C444):
        clip = clip_payloads(8, H, W, siting)
        words = V.block_sad_host(clip[1:], clip[:-1], H, W, siting)
        rep = V.Repeats(*V.dedup_thresholds(True, 8), V.block_counts(H, W, siting))
        print("moving clip, siting %d: max of Y per pair %s (hi = %d)" % (siting, words[:, 0, 0].tolist(), rep.hi))
        assert not any(rep.is_repeat(x) for x in words)
        assert all(a is None for _, a in V.dedup_host(clip, H, W, siting)[0])


# ---- the gap timeline through PassPlanner ---------------------------------------------------------------------------------------------------
def plan_outputs(gaps, rate, dedup_max, pb, cap):
    """What PassPlanner over GapTimeline makes of kept frames with these gaps, the next frame's gap given one frame ahead as RepeatSource
    gives it: [("orig", kept frame) | ("interp", pair's left kept frame, fp32 t)] in write order, and the rows each pass used."""
    tl = V.GapTimeline(rate, dedup_max)
    plan = V.PassPlanner(tl, pb, cap)
    out, used = [], []

    def close(order, pairs, frames_in_slot):
        index = plan.closed_index
        assert len(index) == len(pairs) <= pb
        for kind, row in order:
            if kind == "orig":
                out.append(("orig", frames_in_slot[row]))
            else:
                p, m = divmod(row, tl.slots)
                assert m < len(pairs[p][2])
                out.append(("interp", index[p], pairs[p][2][m]))
        for p, (row, own_left, ts) in enumerate(pairs):
            assert frames_in_slot[row + (1 if own_left else 0)] == index[p] + 1, "the pair's right frame is the row it names"
            assert not own_left or frames_in_slot[row] == index[p]
        used.append(len(frames_in_slot))

    tl.gap(0)
    slot = {}
    for f, g in enumerate(gaps):
        if f + 1 < len(gaps):
            tl.gap(gaps[f + 1])
        slot[plan.rows] = f
        closed = plan.frame()
        if closed is not None:
            close(*closed, slot)
            slot = {}
    close(*plan.end(), slot)
    return out, used, tl


@pytest.mark.parametrize("rate", [1, 2])
@pytest.mark.parametrize("pb", [1, 2])
def test_gap_timeline_through_the_planner(rate, pb):
    gaps = [0, 2, 3, 1, 1, 2, 1, 3]          # kept frames 0 .. 7 sit at input frames 0 2 5 6 7 9 10 13
    out, used, tl = plan_outputs(gaps, rate, 2, pb, 2 * pb + 2)
    assert tl.slots == 3 * rate - 1
    want = [("orig", 0)]
    for i, g in enumerate(gaps[1:]):
        want += [("interp", i, V.Timeline.t32(Fr(j, g * rate))) for j in range(1, g * rate)] + [("orig", i + 1)]
    assert out == want
    assert len(out) == (sum(gaps)) * rate + 1, "the fixed grid's count over the INPUT clip: no row is taken by a repeat, none is lost"
    assert max(used) <= 2 * pb + 2


def test_gap_timeline_alone():
    tl = V.GapTimeline(2, 2, max_slots=5)
    assert tl.slots == 5 and tl.count(0) == 0 and tl.times(0) == []
    tl.gap(0), tl.gap(3)
    assert tl.count(0) == 5 and tl.times(0) == [Fr(j, 6) for j in range(1, 6)]
    assert tl.feed() == [(0, 0)]
    tl.gap(1)
    assert tl.feed() == [(0, Fr(j, 6)) for j in range(1, 6)] + [(1, 0)] and tl.count(1) == 1 and tl.count(2) == 0
    assert tl.feed() == [(1, Fr(1, 2)), (2, 0)]
    assert tl.feed(end=True) == [] and tl.count(0) == 0
    assert V.GapTimeline(1, 1).slots == 1 and V.GapTimeline(8, 2).slots == 23


def test_gap_timeline_refuses_slots_above_the_cap_by_d_and_n():
    with pytest.raises(ValueError, match=r"dedup_max D = 2 at upsample_rate N = 100 puts up to \(D \+ 1\) N - 1 = 299 .* at most 255"):
        V.GapTimeline(100, 2, max_slots=255)
    assert V.GapTimeline(85, 2, max_slots=255).slots == 254
    with pytest.raises(ValueError, match="at least 1"):
        V.GapTimeline(0)


# ---- options ----------------------------------------------------------------------------------------------------------------------------
def test_parse_dedup():
    assert V.parse_dedup(None) is True and V.parse_dedup("") is True and V.parse_dedup(True) is True
    assert V.parse_dedup("768:320:0.33") == (768, 320, Fr(33, 100)) and V.parse_dedup("0:0:0") == (0, 0, 0)
    assert V.parse_dedup(" 12:5:1/3 ") == (12, 5, Fr(1, 3)) and V.parse_dedup((9, 4, Fr(1, 2))) == (9, 4, Fr(1, 2))
    assert V.dedup_thresholds(True, 8) == (768, 320, Fr(33, 100)) and V.dedup_thresholds(None, 10) == (3072, 1280, Fr(33, 100))
    assert V.dedup_thresholds("5:4:1", 16) == (5, 4, 1)
    for bad in ("768:320", "a:b:c", "1:2:3:4", "-1:0:0", "0:-1:0", "0:0:1.5", "0:4194305:0", "1.5:0:0", (1, 2), 7):
        with pytest.raises(ValueError, match="HI:LO:FRAC"):
            V.parse_dedup(bad)
    assert V.parse_dedup("0:4194304:1") == (0, 1 << 22, 1)


class _Model:
    recurrent = False


def _cfg():
    import configparser
    cfg = configparser.RawConfigParser()
    cfg.read_dict({"TRAIN": {"N_FRAMES": "2"}})
    return cfg


def test_interpolator_takes_the_option_and_refuses_what_does_not_go_with_it():
    vi = V.VideoInterpolator(_Model(), _cfg(), upsample_rate=1, dedup=True)
    assert vi.dedup is True and vi.dedup_max == 2 and vi.rate == 1 and vi.repeats == [] and vi.gap_timeline().slots == 2
    vi = V.VideoInterpolator(_Model(), _cfg(), dedup="0:0:0", dedup_max=3, pairs_per_batch=2)
    assert vi.dedup == (0, 0, 0) and vi.rate == 8 and vi.gap_timeline().slots == 31
    assert V.VideoInterpolator(_Model(), _cfg()).dedup is None
    with pytest.raises(ValueError, match="upsample_rate must be at least 2"):
        V.VideoInterpolator(_Model(), _cfg(), upsample_rate=1)          # without the option N = 1 is what it was
    with pytest.raises(ValueError, match="at least 1 with dedup"):
        V.VideoInterpolator(_Model(), _cfg(), upsample_rate=0, dedup=True)
    for name, kw in (("target_rate", dict(target_rate=(60, 1))), ("speed", dict(speed="1/2")), ("shutter", dict(shutter="1/2")),
                     ("scene_cut", dict(scene_cut="1/10")), ("deinterlace", dict(deinterlace="tff"))):
        with pytest.raises(ValueError, match="dedup together with %s is not available.*chain two runs" % name):
            V.VideoInterpolator(_Model(), _cfg(), dedup=True, **kw)
    with pytest.raises(ValueError, match="dedup_max"):
        V.VideoInterpolator(_Model(), _cfg(), dedup=True, dedup_max=0)
    with pytest.raises(ValueError, match=r"D = 2 at upsample_rate N = 43 .* at most 127"):
        V.VideoInterpolator(_Model(), _cfg(), upsample_rate=43, dedup=True, pairs_per_batch=2).gap_timeline()


BASE = ["-c", "x.ini", "--expt", "e", "--log", "l", "--input", "-", "--output", "-"]


def test_cli_flags():
    import interpolate_video as cli
    a = cli.getargs(BASE)
    assert a.dedup is None and a.dedup_max == 2 and a.upsample_rate == 8, "without the flag the tool is as it was"
    a = cli.getargs(BASE + ["--dedup"])
    assert a.dedup is True and a.upsample_rate == 8
    a = cli.getargs(BASE + ["--dedup", "0:0:0", "--dedup_max", "3", "--upsample_rate", "1", "--slowmo", "--detelecine", "--tile", "64x64",
                            "--flow_scale", "1", "--matrix", "bt709", "--range", "full"])
    assert a.dedup == (0, 0, 0) and a.dedup_max == 3 and a.upsample_rate == 1 and a.detelecine


@pytest.mark.parametrize("flags,named", [(["--fps", "60"], "--fps"), (["--speed", "1/2"], "--speed"), (["--speed", "1/2", "--shutter", "180"], "--speed"),
                                         (["--scene_cut", "0.1"], "--scene_cut"), (["--deinterlace", "auto"], "--deinterlace")])
def test_cli_refuses_by_name_and_points_to_two_runs(capsys, flags, named):
    import interpolate_video as cli
    with pytest.raises(SystemExit) as e:
        cli.getargs(BASE + ["--dedup"] + flags)
    assert e.value.code == 2
    assert re.search(r"--dedup does not go together with %s: .* second run" % named, capsys.readouterr().err)


def test_cli_refuses_bad_values(capsys):
    import interpolate_video as cli
    for flags, text in ((["--dedup", "1:2"], "HI:LO:FRAC"), (["--dedup", "--dedup_max", "0"], "dedup_max"),
                        (["--dedup", "--upsample_rate", "0"], "at least 1 with --dedup")):
        with pytest.raises(SystemExit):
            cli.getargs(BASE + flags)
        assert text in capsys.readouterr().err


# ---- ssm_block_sad_fwd: every refusal, nothing queued -----------------------------------------------------------------------------------------
P, Q, OUT = 0x10000, 0x20000, 0x30000          # addresses that are never followed: every call below is refused before anything is queued
FB = 8 * 8 * 3                                # an 8 x 8 frame in 4:4:4 (layout 2)


@pytest.mark.parametrize("args,message", [
    ((None, Q, FB, FB, 1, 8, 8, 2, 1, 0, OUT), "block_sad: null pointer"),
    ((P, None, FB, FB, 1, 8, 8, 2, 1, 0, OUT), "block_sad: null pointer"),
    ((P, Q, FB, FB, 1, 8, 8, 2, 1, 0, None), "block_sad: null pointer"),
    ((P, Q, FB, FB, 0, 8, 8, 2, 1, 0, OUT), "block_sad: N=0 outside 1..65535"),
    ((P, Q, FB, FB, 65536, 8, 8, 2, 1, 0, OUT), "block_sad: N=65536 outside 1..65535"),
    ((P, Q, FB, FB, 1, 0, 8, 2, 1, 0, OUT), "block_sad: bad frame size 0x8"),
    ((P, Q, FB, FB, 1, 8, -1, 2, 1, 0, OUT), "block_sad: bad frame size 8x-1"),
    ((P, Q, FB, FB, 1, 8, 8, 4, 1, 0, OUT), "block_sad: layout 4 not in {0, 1, 2, 3}"),
    ((P, Q, FB, FB, 1, 8, 8, -1, 1, 0, OUT), "block_sad: layout -1 not in {0, 1, 2, 3}"),
    ((P, Q, FB, FB, 1, 8, 8, 2, 0, 0, OUT), "block_sad: sample_bytes 0 not in {1, 2}"),
    ((P, Q, FB, FB, 1, 8, 8, 2, 3, 0, OUT), "block_sad: sample_bytes 3 not in {1, 2}"),
    ((P, Q, FB - 1, FB, 2, 8, 8, 2, 1, 0, OUT), "block_sad: strides 191 (a), 192 (b) neither 0 nor at least the frame's 192 bytes"),
    ((P, Q, FB, 1 - FB, 2, 8, 8, 2, 1, 0, OUT), "block_sad: strides 192 (a), -191 (b) neither 0 nor at least the frame's 192 bytes"),
    ((P, Q, 0, 95, 1, 8, 8, 0, 1, 0, OUT), "block_sad: strides 0 (a), 95 (b) neither 0 nor at least the frame's 96 bytes"),
    ((P + 1, Q, 2 * FB, 2 * FB, 2, 8, 8, 2, 2, 0, OUT), "block_sad: a payload of 2-byte samples (a or b) is not 2-byte aligned"),
    ((P, Q + 1, 2 * FB, 2 * FB, 2, 8, 8, 2, 2, 0, OUT), "block_sad: a payload of 2-byte samples (a or b) is not 2-byte aligned"),
    ((P, Q, 2 * FB + 1, 2 * FB, 2, 8, 8, 2, 2, 0, OUT), "block_sad: strides 385 (a), 384 (b) of 2-byte samples must be even"),
    ((P, Q, FB, FB, 2, 8, 8, 2, 1, -1, OUT), "block_sad: lo=-1 outside 0..2^22"),
    ((P, Q, FB, FB, 2, 8, 8, 2, 1, (1 << 22) + 1, OUT), "block_sad: lo=4194305 outside 0..2^22"),
    ((P, Q, FB, FB, 2, 8, 8, 2, 1, 0, OUT + 4), "block_sad: out is not 8-byte aligned"),
    ((P, Q, 0, 0, 1, 1 << 22, 1 << 22, 2, 1, 0, OUT), "block_sad: a frame of 52776558133248 bytes is more than the grid takes"),
])
def test_block_sad_refusals(args, message):
    from ssm_amd import hipbind as hb
    lib = hb.load()
    assert lib.ssm_block_sad_fwd(*args, None) == -1
    assert lib.ssm_last_error_string().decode() == message


def test_block_sad_refusals_come_in_the_documented_order():
    """A call that is wrong in every way names the first of: pointers, N, H and W, the layout, sample_bytes, strides, 2-byte alignment (the
    addresses, then the strides), lo, out, the grid."""
    from ssm_amd import hipbind as hb
    lib = hb.load()
    err = lambda: lib.ssm_last_error_string().decode()  # noqa: E731
    huge = (1 << 22, 1 << 22)
    f = lib.ssm_block_sad_fwd
    assert f(None, Q + 1, 3, 3, 0, 0, 0, 9, 5, -1, OUT + 4, None) == -1 and "null pointer" in err()
    assert f(P + 1, Q + 1, 3, 3, 0, 0, 0, 9, 5, -1, OUT + 4, None) == -1 and "N=0" in err()
    assert f(P + 1, Q + 1, 3, 3, 2, 0, 0, 9, 5, -1, OUT + 4, None) == -1 and "bad frame size" in err()
    assert f(P + 1, Q + 1, 3, 3, 2, *huge, 9, 5, -1, OUT + 4, None) == -1 and "layout 9" in err()
    assert f(P + 1, Q + 1, 3, 3, 2, *huge, 2, 5, -1, OUT + 4, None) == -1 and "sample_bytes 5" in err()
    assert f(P + 1, Q + 1, 3, 3, 2, *huge, 2, 2, -1, OUT + 4, None) == -1 and "neither 0 nor at least" in err()
    assert f(P + 1, Q + 1, 0, 1 << 50 | 1, 2, *huge, 2, 2, -1, OUT + 4, None) == -1 and "not 2-byte aligned" in err()
    assert f(P, Q, 0, 1 << 50 | 1, 2, *huge, 2, 2, -1, OUT + 4, None) == -1 and "must be even" in err()
    assert f(P, Q, 0, 1 << 50, 2, *huge, 2, 2, -1, OUT + 4, None) == -1 and "lo=-1" in err()
    assert f(P, Q, 0, 1 << 50, 2, *huge, 2, 2, 0, OUT + 4, None) == -1 and "out is not 8-byte aligned" in err()
    assert f(P, Q, 0, 1 << 50, 2, *huge, 2, 2, 0, OUT, None) == -1 and "more than the grid takes" in err()
