"""No-GPU checks of the output timeline of the streamed video path (ssm_amd.video.Timeline, PassPlanner) and of the command line's
--fps / --speed: exact Fractions against hand-written lists, the fixed grid of upsample_rate as the special case step = 1/R, and the
pass bookkeeping of VideoInterpolator._run_timeline replayed on frame numbers instead of payloads."""
from fractions import Fraction as Fr

import numpy as np
import pytest

from ssm_amd import video as V
from ssm_amd.evaluation import t_values

STEPS = (Fr(1, 2), Fr(1, 4), Fr(1, 8), Fr(2, 5), Fr(5, 6), Fr(1200, 1001), Fr(3, 10), Fr(1001, 2500), Fr(6, 5), Fr(5, 2), Fr(1), Fr(2))


@pytest.mark.parametrize("R", [2, 4, 8])
def test_step_one_over_R_is_the_fixed_grid(R):
    tl = V.Timeline(Fr(1, R))
    assert tl.slots == R - 1
    for n in (1, 2, 9):
        assert [(i, t * R) for i, t in tl.outputs(n)] == V.clip_order(n, R)
    want = np.asarray(t_values(R), dtype=np.float32)
    for i in (0, 1, 7):
        got = np.asarray([V.Timeline.t32(t) for t in tl.times(i)], dtype=np.float32)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_30_to_75():
    tl = V.Timeline(V.timeline_step((30, 1), (75, 1)))
    assert tl.step == Fr(2, 5) and tl.slots == 2
    want = [(0, Fr(0)), (0, Fr(2, 5)), (0, Fr(4, 5)), (1, Fr(1, 5)), (1, Fr(3, 5)), (2, Fr(0)), (2, Fr(2, 5)), (2, Fr(4, 5)), (3, Fr(1, 5)),
            (3, Fr(3, 5)), (4, Fr(0))]
    assert tl.outputs(5) == want and len(want) == 11 == tl.n_outputs(5)
    assert [tl.count(i) for i in range(4)] == [2, 2, 2, 2] and tl.times(1) == [Fr(1, 5), Fr(3, 5)]


def test_50_to_60():
    tl = V.Timeline(V.timeline_step((50, 1), (60, 1)))
    assert tl.step == Fr(5, 6) and tl.slots == 1
    out = tl.outputs(6)
    assert len(out) == 7
    assert [i for i, t in out if t == 0] == [0, 5], "only frames 0 and 5 pass through"
    assert [tl.count(i) for i in range(5)] == [1] * 5


def test_ntsc_to_pal_skips_pairs():
    tl = V.Timeline(V.timeline_step((30000, 1001), (25, 1)))
    assert tl.step == Fr(1200, 1001) and tl.slots == 1
    counts = [tl.count(i) for i in range(1200)]
    assert 0 in counts and max(counts) == 1, "some pairs get no frame, none more than one"
    for n in (1, 2, 7, 100, 1201, 1202):
        assert len(tl.outputs(n)) == tl.n_outputs(n) == ((n - 1) * Fr(1001, 1200)).__floor__() + 1


def test_speed():
    """speed = 3/10 at equal rates.  The largest number of frames any pair gets under step 3/10 is 3 (0.3 0.6 0.9 | 1.2 1.5 1.8 |
    2.1 2.4 2.7 | 3.0 is frame 3 itself, and the pattern repeats), not ceil(10/3) = 4: a fourth frame would need a tau within 1/10 after
    an input frame, and the taus are multiples of 3/10 whose fractions are 0, .1 ... .9 with .1 followed by .4, .7 and then 1.0 exactly."""
    assert V.timeline_step((25, 1), None, Fr(3, 10)) == Fr(3, 10) == V.timeline_step((30000, 1001), (30000, 1001), "3/10")
    assert V.timeline_step((24, 1), (60, 1), "0.5") == Fr(1, 5)
    tl = V.Timeline(Fr(3, 10))
    assert tl.slots == 3 == max(sum(1 for i, t in tl.outputs(31) if t and i == p) for p in range(30))
    assert V.Timeline(Fr(3, 11)).slots == 4 == V.Timeline(Fr(3, 11)).count(1)          # 12/11 15/11 18/11 21/11


def test_no_drift():
    tl = V.Timeline(Fr(1001, 2500))
    k = 10 ** 6
    tau = k * Fr(1001, 2500)
    i, t = tl.at(k)
    assert isinstance(t, Fr) and i + t == tau and i == tau.__floor__()
    i, t = tl.at(k + 1)
    assert i + t == tau + Fr(1001, 2500) and 0 <= t < 1


@pytest.mark.parametrize("step", STEPS)
def test_every_output(step):
    tl = V.Timeline(step)
    for n in (1, 2, 5, 12, 40):
        out = tl.outputs(n)
        assert len(out) == ((n - 1) / step).__floor__() + 1
        assert all(0 <= t < 1 for _, t in out)
        assert all(a[0] <= b[0] for a, b in zip(out, out[1:])), "i does not decrease"
        assert all(i + t == k * step for k, (i, t) in enumerate(out))
        assert all(i <= n - 1 and (t == 0 or i + 1 <= n - 1) for i, t in out), "no output needs a frame the clip does not have"
        per_pair = {}
        for i, t in out:
            if t:
                per_pair[i] = per_pair.get(i, 0) + 1
        assert all(tl.count(i) == per_pair.get(i, 0) for i in range(n - 1))
        assert max(per_pair.values(), default=0) <= tl.slots
    assert tl.slots == max([tl.count(i) for i in range(step.numerator)])


@pytest.mark.parametrize("step", STEPS)
def test_feed_equals_outputs(step):
    tl = V.Timeline(step)
    for n in range(1, 13):
        got = []
        for f in range(n):
            new = tl.feed()
            assert all(i + (1 if t else 0) == f for i, t in new), "an output comes with the frame that completes it, not later"
            got += new
        assert tl.feed(end=True) == []
        assert got == tl.outputs(n)


@pytest.mark.parametrize("bad", [0, Fr(-1, 3), "-2/5"])
def test_non_positive_step_is_refused(bad):
    with pytest.raises(ValueError, match="got %s" % Fr(bad)):
        V.Timeline(bad)


def test_unparsable_values_are_named():
    for bad in ("sixty", "60:", "60:0", "0", "-24", "59.94"):
        with pytest.raises(ValueError, match=repr(bad)):
            V.parse_rate(bad)
    assert V.parse_rate("60") == (60, 1) and V.parse_rate("60000:1001") == (60000, 1001) and V.parse_rate("50:2") == (50, 2)
    for bad in ("fast", "1/0", "0", "-0.5", ""):
        with pytest.raises(ValueError, match=repr(bad)):
            V.parse_speed(bad)
    assert V.parse_speed("0.25") == V.parse_speed("1/4") == Fr(1, 4) and V.parse_speed("3/10") == Fr(3, 10) == V.parse_speed(Fr(3, 10))


def test_slots_beyond_the_plan_are_refused():
    with pytest.raises(ValueError, match="at most 255"):
        V.Timeline(Fr(1, 257), max_slots=V.MAX_STAGE2_BATCH)
    assert V.Timeline(Fr(1, 256), max_slots=V.MAX_STAGE2_BATCH).slots == 255


class _Cfg:
    def getint(self, section, key):
        return 2


def test_interpolator_arguments():
    vi = V.VideoInterpolator(None, _Cfg(), target_rate=(75, 1))
    assert vi.timed and vi.timeline((30, 1)).step == Fr(2, 5)
    vi = V.VideoInterpolator(None, _Cfg(), speed="3/10", pairs_per_batch=2)
    assert vi.timed and vi.timeline((30000, 1001)).step == Fr(3, 10)
    with pytest.raises(ValueError, match="at most 127"):
        V.VideoInterpolator(None, _Cfg(), speed=Fr(1, 200), pairs_per_batch=2).timeline((25, 1))
    assert not V.VideoInterpolator(None, _Cfg()).timed
    with pytest.raises(ValueError, match="'0'"):
        V.VideoInterpolator(None, _Cfg(), speed="0")
    with pytest.raises(ValueError, match="0:1"):
        V.VideoInterpolator(None, _Cfg(), target_rate=(0, 1))


# ---- the pass bookkeeping, replayed on frame numbers ------------------------------------------------------------------------------
def replay(step, n, pb, cap):
    """What _run_timeline does with a PassPlanner, with a frame's number in place of its payload: returns the written (i, fp32 t) and
    the frames that were uploaded, in order."""
    tl = V.Timeline(step)
    S = tl.slots
    plan = V.PassPlanner(V.Timeline(step), pb, cap)
    written, uploaded, right = [], [], [None]

    def close(order, pairs, slot):
        assert len(pairs) <= pb
        made = {}
        for p, (row, own_left, ts) in enumerate(pairs):
            assert 1 <= len(ts) <= S
            if own_left:
                left, new = slot[row], [slot[row], slot[row + 1]]
            else:
                left, new = right[0], [slot[row]]
            uploaded.extend(new)
            assert new[-1] == left + 1, "a pair is two neighbouring frames"
            right[0] = new[-1]
            for q, t in enumerate(ts):
                made[p * S + q] = (left, t)
        for kind, row in order:
            written.append(made[row] if kind == "interp" else (slot[row], np.float32(0)))

    slot = [None] * cap
    for f in range(n):
        slot[plan.rows] = f
        closed = plan.frame()
        if closed is not None:
            close(*closed, slot)
            slot = [None] * cap
    close(*plan.end(), slot)
    return written, uploaded


@pytest.mark.parametrize("step", STEPS + (Fr(7, 3), Fr(1001, 1000)))
def test_pass_planner_writes_the_timeline_and_uploads_each_needed_frame_once(step):
    tl = V.Timeline(step)
    for n in list(range(1, 14)) + [40]:
        want = [(i, V.Timeline.t32(t)) for i, t in tl.outputs(n)]
        needed = sorted({j for i, t in tl.outputs(n) if t for j in (i, i + 1)})
        for pb in (1, 2, 3):
            for cap in (2, 3, 2 * pb + 2):
                written, uploaded = replay(step, n, pb, cap)
                assert written == want, (step, n, pb, cap)
                assert uploaded == needed, "every frame a synthesised output needs goes up once, no other does"


# ---- command line ------------------------------------------------------------------------------------------------------------------
BASE = ["-c", "x.ini", "--expt", "e", "--log", "l", "--input", "-", "--output", "-"]


def test_cli_flags():
    import interpolate_video as cli
    a = cli.getargs(BASE)
    assert a.upsample_rate == 8 and a.fps is None and a.speed is None, "with neither flag the tool is as it was"
    assert cli.getargs(BASE + ["--upsample_rate", "3"]).upsample_rate == 3
    a = cli.getargs(BASE + ["--fps", "60000:1001"])
    assert a.fps == (60000, 1001) and a.speed is None
    assert cli.getargs(BASE + ["--fps", "75"]).fps == (75, 1)
    for text in ("0.25", "1/4"):
        a = cli.getargs(BASE + ["--speed", text])
        assert a.speed == Fr(1, 4) and a.fps is None
    a = cli.getargs(BASE + ["--fps", "60", "--speed", "3/10"])
    assert a.fps == (60, 1) and a.speed == Fr(3, 10)


@pytest.mark.parametrize("extra,named", [(["--fps", "75", "--upsample_rate", "4"], "--upsample_rate"),
                                         (["--speed", "1/4", "--upsample_rate", "8"], "--upsample_rate"),
                                         (["--fps", "75", "--slowmo"], "--slowmo"),
                                         (["--fps", "sixty"], "'sixty'"), (["--speed", "fast"], "'fast'"), (["--speed", "0"], "'0'")])
def test_cli_errors(capsys, extra, named):
    import interpolate_video as cli
    with pytest.raises(SystemExit) as e:
        cli.getargs(BASE + extra)
    assert e.value.code == 2
    assert named in capsys.readouterr().err
