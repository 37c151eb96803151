"""No-GPU checks of the shutter of the streamed video path: Timeline(step, shutter=, samples=) against a brute-force enumeration in
Fractions, the pass bookkeeping of VideoInterpolator._run_shutter (ssm_amd.video.ShutterPlanner) replayed on frame numbers instead of
payloads, the numpy yardstick of the accumulation kernel against a float64 sum, and the command line's --shutter."""
import math
from fractions import Fraction as Fr

import numpy as np
import pytest

from ssm_amd import video as V

# (step, sigma, S): samples that span pairs and skip pairs; samples that are input frames; an NTSC-like step with an odd shutter; a
# slow-motion step whose pairs get up to 7 samples
CASES = [(Fr(5, 2), Fr(1, 2), 4), (Fr(1, 2), Fr(1), 3), (Fr(1001, 400), Fr(12, 25), 5), (Fr(3, 10), Fr(1), 2)]
IDS = ["5/2-180deg-4", "1/2-360deg-3", "1001/400-172.8deg-5", "3/10-360deg-2"]
N_MAX = 40


def brute(step, sigma, S, n):
    """The definition, enumerated: [tuple of the S (i, t) of output k] for every k whose last sample lies at n - 1 or before."""
    outs, k = [], 0
    while True:
        taus = [k * step + j * (sigma * step / S) for j in range(S)]
        if taus[-1] > n - 1:
            return outs
        outs.append(tuple((math.floor(tau), tau - math.floor(tau)) for tau in taus))
        k += 1


def brute_pairs(step, sigma, S, n_pairs):
    """{pair i: [(t, k, j)] of its synthesised samples in time order}, {frame i: (k, j) of the sample that is the frame itself}."""
    synth, frames, k = {i: [] for i in range(n_pairs)}, {}, 0
    while k * step < n_pairs:
        for j in range(S):
            tau = k * step + j * (sigma * step / S)
            i = math.floor(tau)
            if tau == i:
                frames[i] = (k, j)
            elif i < n_pairs:
                synth[i].append((tau - i, k, j))
        k += 1
    return synth, frames


@pytest.mark.parametrize("step,sigma,S", CASES, ids=IDS)
def test_timeline_against_brute_force(step, sigma, S):
    tl = V.Timeline(step, shutter=sigma, samples=S)
    assert (tl.step, tl.shutter, tl.samples) == (step, sigma, S)
    for n in range(1, N_MAX + 1):
        want = brute(step, sigma, S, n)
        assert tl.n_outputs(n) == len(want), n
        assert tl.outputs(n) == want, n
        assert all(tl.samples_of(k) == list(want[k]) for k in range(len(want)))
        got = []
        for f in range(n):
            new = tl.feed()
            for smp in new:
                i, t = smp[-1]
                assert i + (1 if t else 0) == f, "an output comes with the frame that completes its last sample, not later"
            got += new
        assert tl.feed(end=True) == []
        assert got == want, "feed() piece by piece is outputs(n)"
    assert tl.n_outputs(0) == 0
    period = step.numerator
    synth, frames = brute_pairs(step, sigma, S, max(N_MAX, 2 * period))
    for i, want in synth.items():
        assert tl.count(i) == len(want), i
        assert tl.times(i) == want, i
        assert tl.on_frame(i) == frames.get(i), i
        assert all(0 < t < 1 for t, _, _ in want) and want == sorted(want)
    assert tl.slots == max(len(synth[i]) for i in range(period)), "slots is the maximum over one period"
    assert tl.slots == max(len(v) for v in synth.values()), "and a second period holds no more"


@pytest.mark.parametrize("step", [Fr(1, 2), Fr(2, 5), Fr(5, 6), Fr(1200, 1001), Fr(3, 10), Fr(5, 2), Fr(1), Fr(2)])
def test_one_sample_is_the_timeline_without_a_shutter(step):
    for sigma in (None, Fr(1, 2), 1):
        a, b = V.Timeline(step), V.Timeline(step, shutter=sigma, samples=1)
        assert b.slots == a.slots
        for n in (1, 2, 7, N_MAX):
            assert b.outputs(n) == a.outputs(n) and b.n_outputs(n) == a.n_outputs(n)
            got = [x for _ in range(n) for x in b.feed()]
            b.feed(end=True)
            assert got == a.outputs(n)
        for i in range(N_MAX):
            assert b.count(i) == a.count(i) and b.times(i) == a.times(i)
            assert (b.on_frame(i) is not None) == any(j == i and not t for j, t in a.outputs(N_MAX + 1))
        assert all(b.samples_of(k) == [a.at(k)] for k in range(20))


@pytest.mark.parametrize("bad", [0, Fr(-1, 2), Fr(3, 2), "1.25"])
def test_shutter_outside_its_interval_is_refused(bad):
    with pytest.raises(ValueError, match=r"\(0, 1\] \(got %s\)" % Fr(bad)):
        V.Timeline(Fr(5, 2), shutter=bad, samples=4)
    with pytest.raises(ValueError, match=r"got %s\)" % Fr(bad)):
        V.VideoInterpolator(None, _Cfg(), speed=Fr(5, 2), shutter=bad)


@pytest.mark.parametrize("bad", [0, -3, 2.5])
def test_sample_counts_below_one_are_refused(bad):
    with pytest.raises(ValueError, match=r"at least 1 \(got %r\)" % (bad,)):
        V.Timeline(Fr(5, 2), shutter=Fr(1, 2), samples=bad)
    with pytest.raises(ValueError, match=r"got %r\)" % (bad,)):
        V.VideoInterpolator(None, _Cfg(), speed=Fr(5, 2), shutter=Fr(1, 2), shutter_samples=bad)


class _Cfg:
    def getint(self, section, key):
        return 2


def test_slots_beyond_the_plan_are_refused():
    """step 1/16 with 16 samples over the whole interval puts 255 sub-frames between two input frames (every multiple of 1/256 but the
    frame itself): the most one pair per pass takes, and too many for two."""
    assert V.Timeline(Fr(1, 16), max_slots=V.MAX_STAGE2_BATCH, shutter=1, samples=16).slots == 255
    vi = V.VideoInterpolator(None, _Cfg(), speed=Fr(1, 16), shutter=1, shutter_samples=16)
    assert vi.timed and vi.timeline((25, 1)).slots == 255
    with pytest.raises(ValueError, match="255 sub-frames.*at most 127"):
        V.VideoInterpolator(None, _Cfg(), speed=Fr(1, 16), shutter=1, shutter_samples=16, pairs_per_batch=2).timeline((25, 1))
    with pytest.raises(ValueError, match="511 sub-frames.*at most 255"):
        V.Timeline(Fr(1, 16), max_slots=V.MAX_STAGE2_BATCH, shutter=1, samples=32)


def test_interpolator_arguments():
    vi = V.VideoInterpolator(None, _Cfg(), target_rate=(24, 1), shutter="1/2")
    tl = vi.timeline((60, 1))
    assert vi.timed and (tl.step, tl.shutter, tl.samples) == (Fr(5, 2), Fr(1, 2), 8), "8 samples unless told otherwise"
    vi = V.VideoInterpolator(None, _Cfg(), target_rate=(24, 1), shutter=Fr(1, 2), shutter_samples=1)
    assert vi.timed and vi.samples == 1 and vi.timeline((60, 1)).samples == 1
    with pytest.raises(ValueError, match="give one of them"):
        V.VideoInterpolator(None, _Cfg(), shutter=Fr(1, 2))          # as the command line: a shutter needs the timeline of a rate or a speed
    assert V.VideoInterpolator(None, _Cfg(), speed=1, shutter=Fr(1, 2)).timeline((25, 1)).step == 1
    vi = V.VideoInterpolator(None, _Cfg(), shutter_samples=4)
    assert not vi.timed and vi.samples == 1, "without a shutter the sample count means nothing"
    assert V.parse_shutter("180") == Fr(1, 2) and V.parse_shutter("172.8") == Fr(12, 25) and V.parse_shutter("90") == Fr(1, 4)
    assert V.parse_shutter("360") == 1 and V.parse_shutter(Fr(45)) == Fr(1, 8)
    for bad in ("0", "400", "-90", "wide", ""):
        with pytest.raises(ValueError, match=repr(bad)):
            V.parse_shutter(bad)


# ---- the pass bookkeeping, replayed on frame numbers ------------------------------------------------------------------------------
def replay(step, sigma, S, n, pb, cap):
    """What _run_shutter does with a ShutterPlanner, with a frame's number in place of its payload and a list in place of an accumulator.
    Returns the written outputs as [(k, [(frame i, fp32 t)] in the order they were added)] and the uploaded frames in order."""
    tl = V.Timeline(step, shutter=sigma, samples=S)
    plan = V.ShutterPlanner(tl, pb, cap)
    slots = tl.slots
    written, uploaded = [], []
    acc = [None] * V.OPEN_OUTPUTS                 # per accumulator: None (free: never used, or handed to the writer), or [k, samples]
    prev_planes = [None]

    def close(rows, carry, pairs, calls, done, slot):
        planes = [None] * (cap + 1)
        if carry is not None:
            planes[0] = prev_planes[0][carry]
            assert planes[0] is not None
        assert 0 <= rows <= cap
        planes[1:1 + rows] = slot[:rows]
        uploaded.extend(slot[:rows])
        assert len(pairs) <= pb
        made = {}
        for p, (left, right, ts) in enumerate(pairs):
            assert 1 <= len(ts) <= slots
            assert planes[right] == planes[left] + 1, "a pair is two neighbouring frames"
            for q, t in enumerate(ts):
                made[p * slots + q] = (planes[left], t)
        finished = []
        for src, first, count, k, init, last in calls:
            if src == "frame":
                assert count == 1 and planes[first] is not None
                frames = [(planes[first], np.float32(0))]
            else:
                assert first // slots == (first + count - 1) // slots, "one call stays within one pair"
                frames = [made[first + q] for q in range(count)]
            a = k % V.OPEN_OUTPUTS
            if init:
                assert acc[a] is None, "an accumulator is initialised again only after its output went to the writer"
                acc[a] = [k, []]
            assert acc[a] is not None and acc[a][0] == k, "a call without init finds its own output's sum"
            acc[a][1].extend(frames)
            assert sum(x is not None for x in acc) <= V.OPEN_OUTPUTS
            if last:
                finished.append(k)
                written.append((k, acc[a][1]))
                acc[a] = None
        assert finished == list(done) and len(done) <= plan.max_done
        if rows:
            prev_planes[0] = planes

    slot = [None] * cap
    for f in range(n):
        slot[plan.rows] = f
        closed = plan.frame()
        if closed is not None:
            close(*closed, slot)
            slot = [None] * cap
    close(*plan.end(), slot)
    return written, uploaded


@pytest.mark.parametrize("pb", [1, 2, 3])
@pytest.mark.parametrize("step,sigma,S", CASES, ids=IDS)
def test_planner_gives_every_output_its_samples_in_time_order(step, sigma, S, pb):
    tl = V.Timeline(step, shutter=sigma, samples=S)
    for n in range(1, N_MAX + 1):
        want = [(k, [(i, V.Timeline.t32(t)) for i, t in smp]) for k, smp in enumerate(brute(step, sigma, S, n))]
        # a frame is needed when a sample at n - 1 or before is that frame or lies between it and a neighbour; the planner cannot know
        # where a pipe ends, so this counts the samples of an output that the end of the clip cuts short as well
        needed, k = set(), 0
        while k * step <= n - 1:
            for i, t in tl.samples_of(k):
                if i + t <= n - 1:
                    needed.update([i] if not t else [i, i + 1])
            k += 1
        for cap in (2, 3, 2 * pb + 2):
            written, uploaded = replay(step, sigma, S, n, pb, cap)
            assert [k for k, _ in written] == list(range(len(want))), "the writer takes the outputs in order of k"
            assert written == want, (n, pb, cap)
            assert uploaded == sorted(needed), "every frame a sample needs goes up once, no other does"


def test_planner_marks_init_and_scale_once_per_output():
    """Case (a) of the GPU test, spelled out: 60 -> 24 at 180 degrees in 4 samples, 9 frames, one pair per pass."""
    tl = V.Timeline(Fr(5, 2), shutter=Fr(1, 2), samples=4)
    plan = V.ShutterPlanner(tl, 1, 4)
    passes = [c for c in (plan.frame() for _ in range(9)) if c is not None] + [plan.end()]
    calls = [c for _, _, _, cs, _ in passes for c in cs]
    # taus: 0 5/16 10/16 15/16 | 2.5 2.8125 3.125 3.4375 | 5 5.3125 5.625 5.9375 | 7.5 7.8125 (8.125 and 8.4375 are past frame 8)
    assert [(c[0], c[2], c[3], c[4], c[5]) for c in calls] == [
        ("frame", 1, 0, True, False), ("interp", 3, 0, False, True),
        ("interp", 2, 1, True, False), ("interp", 2, 1, False, True),
        ("frame", 1, 2, True, False), ("interp", 3, 2, False, True),
        ("interp", 2, 3, True, False)]
    assert [k for p in passes for k in p[4]] == [0, 1, 2] == list(range(tl.n_outputs(9)))
    assert sum(1 for p in passes if p[2]) == 5, "pairs 0, 2, 3, 5 and 7 run, 7 for an output that the end of the clip cuts short; 1, 4 and 6 do not"


# ---- the yardstick of the kernel ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 7, 16])
@pytest.mark.parametrize("init", [0, 1])
def test_accumulate_host_against_float64(n, init):
    """s_0 = a + x_0 (or x_0), s_m = s_(m-1) + x_m, out = s * scale, each rounded to fp32: with u = 2^-24 every addition errs by at most
    u |s_m| <= u A for A = |a| + sum |x|, the product by u |s scale|, so |out - exact| <= ((adds + 1) u (1 + u)^adds) A |scale|."""
    rng = np.random.default_rng(100 * n + init)
    shape = (n, 3, 9, 11)
    x = (rng.standard_normal(shape) * 10.0 ** rng.uniform(-3, 3, shape)).astype(np.float32)
    a0 = (rng.standard_normal(shape[1:]) * 10.0 ** rng.uniform(-3, 3, shape[1:])).astype(np.float32)
    for scale in (1.0, np.float32(1.0 / 3.0), 0.125):
        acc = a0.copy()[None]
        out = V.accumulate_host(x, acc, init, scale)
        assert out is acc and out.dtype == np.float32 and out.shape == (1,) + shape[1:]
        exact = (x.astype(np.float64).sum(0) + (0 if init else a0.astype(np.float64))) * float(np.float32(scale))
        mag = np.abs(x.astype(np.float64)).sum(0) + (0 if init else np.abs(a0.astype(np.float64)))
        adds = n - 1 + (0 if init else 1)
        u = 2.0 ** -24
        bound = (adds + 1) * u * (1 + u) ** adds * mag * float(np.float32(scale))
        assert np.all(np.abs(out[0].astype(np.float64) - exact) <= bound), float(np.max(np.abs(out[0] - exact) - bound))
    # the order is the kernel's: left to right from the accumulator, one rounding per step
    s = x[0] if init else a0 + x[0]
    for m in range(1, n):
        s = s + x[m]
    assert np.array_equal(V.accumulate_host(x, a0.copy(), init, np.float32(1.0 / 3.0)), s * np.float32(1.0 / 3.0))


# ---- command line ------------------------------------------------------------------------------------------------------------------
BASE = ["-c", "x.ini", "--expt", "e", "--log", "l", "--input", "-", "--output", "-"]


def test_cli_flags():
    import interpolate_video as cli
    a = cli.getargs(BASE)
    assert a.shutter is None and a.upsample_rate == 8, "without the flag the tool is as it was"
    a = cli.getargs(BASE + ["--fps", "24", "--shutter", "180"])
    assert a.shutter == Fr(1, 2) and a.shutter_samples == 8 and a.fps == (24, 1)
    a = cli.getargs(BASE + ["--speed", "5/2", "--shutter", "172.8", "--shutter_samples", "5"])
    assert a.shutter == Fr(12, 25) and a.shutter_samples == 5
    assert cli.getargs(BASE + ["--fps", "24", "--shutter", "360"]).shutter == 1
    assert cli.getargs(BASE + ["--fps", "24", "--shutter", "90"]).shutter == Fr(1, 4)


@pytest.mark.parametrize("extra,named", [(["--shutter", "180"], "it needs one of them"),
                                         (["--shutter", "180", "--upsample_rate", "4"], "it needs one of them, and does not go together with"),
                                         (["--fps", "24", "--shutter", "180", "--upsample_rate", "4"],
                                          "--fps / --speed / --shutter set the output's timeline themselves: they do not go together"),
                                         (["--fps", "24", "--shutter", "180", "--slowmo"],
                                          "--fps / --speed / --shutter set the output's timeline themselves: they do not go together"),
                                         (["--fps", "24", "--shutter", "0"], "'0'"), (["--fps", "24", "--shutter", "400"], "'400'"),
                                         (["--fps", "24", "--shutter", "180", "--shutter_samples", "0"], "got 0")])
def test_cli_errors(capsys, extra, named):
    import interpolate_video as cli
    with pytest.raises(SystemExit) as e:
        cli.getargs(BASE + extra)
    assert e.value.code == 2
    assert named in capsys.readouterr().err, "the error is the intended refusal, not another parse failure (the usage line names every flag)"
