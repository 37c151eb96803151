"""The per-block fallback as a cross-fade without a GPU: ssm_amd.video.flow_mix_host against a loop written out block by
block and sample by sample in Fractions, floor(x + 1/2) of the exact a (1 - t) + b t; that the fraction which names t does not matter; the
two ends against flow_paste_host; the kernel's division (video_score.mix_divisor) against // over the numerators a den up to 65535 can
reach; how a pair's times become three launch scalars; the refusals of the option flow_fallback in VideoInterpolator and in
scripts/interpolate_video.py; and the SSM_E_ARG refusals of ssm_flow_mix_fwd, in their order, through the loaded library.  Everything
compared is exact."""
import math
import os
import sys
import types
from fractions import Fraction as Fr

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_flow_repair_cpu as R  # noqa: E402
import video_option_cases as C  # noqa: E402
from video_clips import LAYOUTS  # noqa: E402
from ssm_amd import video as V  # noqa: E402
from ssm_amd import video_score as VS  # noqa: E402

N = R.N
# (num0, num_step, den) and the most outputs whose k_j = num0 + j num_step stay in 0 .. den (at most 7, the fixed grid of rate 8)
TRIPLES = (((1, 1, 2), 2), ((1, 1, 3), 3), ((1, 1, 8), 7), ((2, 2, 5), 2), ((400, 0, 1000), 3), ((77, 308, 1001), 4), ((1, 65533, 65535), 2))
SIZES = ((16, 24), (17, 23), (9, 25))
KS = (20, 0, 63)


# ---- the yardstick against a loop ----------------------------------------------------------------------------------------------------------
def operands(h, w, layout, bits, t, seed):
    rng = np.random.RandomState(seed)
    fb = V.frame_bytes(h, w, layout, bits)
    a, b = (rng.randint(0, 256, size=(N, fb + 3)).astype(np.uint8) for _ in range(2))
    outputs = rng.randint(0, 256, size=(N, t, fb + 5)).astype(np.uint8)
    return a, b, outputs


def by_loop(outputs, a, b, mask, h, w, layout, bits, k, num0, num_step, den):
    """The definition, one block and one sample at a time: x = a (1 - t) + b t at the Fraction t = k_j / den, then floor(x + 1/2)."""
    sb = V.sample_bytes(bits)
    fb = V.frame_bytes(h, w, layout, bits)
    res, counts = outputs.copy(), [0] * outputs.shape[0]
    planes, sub = R.plane_offsets(h, w, layout)
    for n in range(outputs.shape[0]):
        for by in range(h >> 3):
            for bx in range(w >> 3):
                bad = 0
                for y in range(8 * by, 8 * by + 8):
                    for x in range(8 * bx, 8 * bx + 8):
                        bad += (int(mask[n, 0, y, x]) | int(mask[n, 1, y, x])) & 1
                if bad <= k:
                    continue
                counts[n] += 1
                for p, (rows, cols, first) in enumerate(planes):
                    rr, rc = (8, 8) if p == 0 else sub
                    for y in range(rr * by, rr * by + rr):
                        for x in range(rc * bx, rc * bx + rc):
                            o = (first + y * cols + x) * sb
                            assert y < rows and x < cols and o + sb <= fb
                            va, vb = (int.from_bytes(src[n, o:o + sb].tobytes(), "little") for src in (a, b))
                            for j in range(outputs.shape[1]):
                                t = Fr(num0 + j * num_step, den)
                                assert 0 <= t <= 1
                                v = math.floor(va * (1 - t) + vb * t + Fr(1, 2))
                                res[n, j, o:o + sb] = np.frombuffer(v.to_bytes(sb, "little"), np.uint8)
    return res, counts


@pytest.mark.parametrize("bits", [8, 10, 16])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_yardstick_equals_the_loop(layout, bits):
    for idx, ((num0, num_step, den), t) in enumerate(TRIPLES):
        h, w = SIZES[(idx + layout) % len(SIZES)]
        k = KS[(idx + bits) % len(KS)]
        a, b, outputs = operands(h, w, layout, bits, t, seed=h * w + layout + bits + idx)
        mask, planted = R.planted_mask(h, w, k, seed=k + h)
        got, counts = V.flow_mix_host(outputs, a, b, mask, h, w, layout, bits, k, num0, num_step, den)
        want, want_counts = by_loop(outputs, a, b, mask, h, w, layout, bits, k, num0, num_step, den)
        assert counts.dtype == np.uint64 and counts.tolist() == want_counts, (h, w, k, den)
        assert np.array_equal(got, want), (h, w, k, den)
        _, paste_counts = V.flow_paste_host(outputs, a, b, mask, h, w, layout, bits, k, 1)
        assert counts.tolist() == paste_counts.tolist(), "the blocks, the test and the counts are flow_paste_host's"
        fail = V.flow_block_counts_host(mask, h, w) > k
        assert not fail[0].reshape(-1)[0], "n = K passes"
        if 1 in planted:
            assert fail[0].reshape(-1)[1], "n = K + 1 in direction 1 alone fails"
        assert sum(want_counts) > 0 and not np.array_equal(got, outputs), "something is mixed"


def test_a_frame_without_blocks_and_a_k_that_fails_nothing():
    for h, w in ((7, 40), (40, 7)):
        a, b, outputs = operands(h, w, V.C444, 8, 3, seed=1)
        got, counts = V.flow_mix_host(outputs, a, b, np.ones((N, 2, h, w), np.uint8), h, w, V.C444, 8, 0, 1, 1, 4)
        assert np.array_equal(got, outputs) and counts.tolist() == [0, 0]
    a, b, outputs = operands(16, 24, V.C422, 16, 3, seed=2)
    got, counts = V.flow_mix_host(outputs, a, b, np.ones((N, 2, 16, 24), np.uint8), 16, 24, V.C422, 16, 64, 1, 1, 4)
    assert np.array_equal(got, outputs) and counts.tolist() == [0, 0], "K = 64 changes nothing"


@pytest.mark.parametrize("bits", [8, 10, 16])
def test_the_fraction_that_names_t_does_not_matter(bits):
    """2/5 and 400/1000, 1/3 and 21845/65535, 7/8 and 875/1000: the exact rational rounded half up is one value."""
    h, w, layout = 16, 24, V.C422
    mask = np.ones((N, 2, h, w), np.uint8)
    for (p, q), (p2, q2) in (((2, 5), (400, 1000)), ((1, 3), (21845, 65535)), ((7, 8), (875, 1000)), ((1, 2), (500, 1000))):
        assert Fr(p, q) == Fr(p2, q2)
        a, b, outputs = operands(h, w, layout, bits, 1, seed=p + q)
        one, _ = V.flow_mix_host(outputs, a, b, mask, h, w, layout, bits, 0, p, 0, q)
        two, _ = V.flow_mix_host(outputs, a, b, mask, h, w, layout, bits, 0, p2, 0, q2)
        assert np.array_equal(one, two) and not np.array_equal(one, outputs)
    # an arithmetic progression named twice: 2/5, 4/5 over 5 and over 1000
    a, b, outputs = operands(h, w, layout, bits, 2, seed=9)
    one, _ = V.flow_mix_host(outputs, a, b, mask, h, w, layout, bits, 0, 2, 2, 5)
    two, _ = V.flow_mix_host(outputs, a, b, mask, h, w, layout, bits, 0, 400, 400, 1000)
    assert np.array_equal(one, two)


@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_the_ends_are_the_frames_themselves(layout, bits):
    """k_j = 0 is flow_paste_host with split = T (a everywhere), k_j = den with split = 0 (b everywhere)."""
    h, w, t, k = 17, 23, 3, 20
    a, b, outputs = operands(h, w, layout, bits, t, seed=layout + bits)
    mask, _ = R.planted_mask(h, w, k, seed=4)
    for den in (2, 1001, 65535):
        for num0, split in ((0, t), (den, 0)):
            got, counts = V.flow_mix_host(outputs, a, b, mask, h, w, layout, bits, k, num0, 0, den)
            want, want_counts = V.flow_paste_host(outputs, a, b, mask, h, w, layout, bits, k, split)
            assert np.array_equal(got, want) and counts.tolist() == want_counts.tolist() and sum(counts.tolist()) > 0


def test_ten_bit_codes_stay_ten_bit_and_the_largest_numerator():
    h, w, layout = 16, 24, V.CENTRED
    fb, mask = V.frame_bytes(h, w, layout, 10), np.ones((1, 2, h, w), np.uint8)
    rng = np.random.RandomState(5)
    a, b = (rng.randint(0, 1024, size=(1, fb // 2)).astype("<u2") for _ in range(2))
    a[0, :4], b[0, :4] = (1023, 0, 1023, 1022), (0, 1023, 1023, 1023)
    outputs = np.zeros((1, 7, fb), np.uint8)
    got, _ = V.flow_mix_host(outputs, a.view(np.uint8), b.view(np.uint8), mask, h, w, layout, 10, 0, 1, 1, 8)
    words = got.view("<u2")
    assert words.max() == 1023 and words[0, :, 2].tolist() == [1023] * 7, "a mix of two codes <= 1023 is <= 1023"
    assert words[0, :, 0].tolist() == [(1023 * (8 - j) + 4) // 8 for j in range(1, 8)]
    # den = 65535 with the words 0 and 65535: the numerator 65535 * 65535 + 32767, the largest there is
    a16, b16 = np.full((1, fb // 2), 65535, "<u2"), np.zeros((1, fb // 2), "<u2")
    b16[0, ::2] = 65535
    got, _ = V.flow_mix_host(outputs[:, :2], a16.view(np.uint8), b16.view(np.uint8), mask, h, w, layout, 16, 0, 1, 65533, 65535)
    words = got.view("<u2")
    assert (words[0, :, ::2] == 65535).all() and words[0, 0, 1] == 65534 and words[0, 1, 1] == 1


# ---- the kernel's division ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("den", [2, 3, 5, 1001, 2500, 4096, 65521, 65535])
def test_mix_divisor_is_exact_on_the_numerators_a_mix_reaches(den):
    """a (den - k) + b k + den // 2 for the extreme samples and weights, and the multiples of den beside each, one below and one above:
    where a quotient steps."""
    xs = set()
    for a in (0, 1, 65534, 65535):
        for b in (0, 1, 65534, 65535):
            for k in (0, 1, den // 2, den - 1, den):
                x = a * (den - k) + b * k + den // 2
                xs.add(x)
                for m in (x // den, x // den + 1):
                    xs.update(m * den + e for e in (-1, 0, 1))
    xs = sorted(x for x in xs if 0 <= x < 1 << 32)
    assert xs[-1] >= 65535 * den + den // 2, "the largest numerator of this den is among them"
    m, shift = VS.mix_divisor(den)
    assert 0 < m < 1 << 32 and shift == (den - 1).bit_length() - 1
    assert VS.mix_divide(np.array(xs, np.uint64), den).tolist() == [x // den for x in xs]


# ---- a pair's times as three launch scalars ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", range(2, 10))
def test_scalars_of_the_fixed_grid(rate):
    times = [Fr(j, rate) for j in range(1, rate)]
    assert V.fixed_mix(rate) == (1, 1, rate) and V.times_mix(times, rate) == (1, 1 if rate > 2 else 0, rate), "one output: the step is 0"
    num0, num_step, den = V.fixed_mix(rate)
    assert [Fr(num0 + j * num_step, den) for j in range(rate - 1)] == times


@pytest.mark.parametrize("in_rate, target, den", [((24000, 1001), (60000, 1001), 5), ((24, 1), (60000, 1001), 2500),
                                                  ((30000, 1001), (25, 1), 1001), ((240, 1), (640, 1), 8), ((240, 1), (600, 1), 5)])
def test_scalars_of_a_timeline(in_rate, target, den):
    tl = V.Timeline(V.timeline_step(in_rate, target))
    assert V.flow_mix_den(tl) == den == tl.step.denominator
    seen = 0
    for i in range(40):
        times = tl.times(i)
        if not times:
            continue
        num0, num_step, d = V.times_mix(times, den)
        assert d == den and [Fr(num0 + j * num_step, den) for j in range(len(times))] == times, "the kernel's k_j / den are the exact times"
        assert num_step == (tl.step.numerator if len(times) > 1 else 0)
        seen += 1
    assert seen > 5
    with pytest.raises(AssertionError, match="step evenly"):
        V.times_mix([Fr(1, 8), Fr(2, 8), Fr(4, 8)], 8)
    with pytest.raises(AssertionError, match="whole numbers over den"):
        V.times_mix([Fr(1, 3)], 8)


def test_a_denominator_above_the_limit_is_refused_by_name():
    for step in (Fr(1, 65536), Fr(333333, 1000000)):
        with pytest.raises(ValueError) as e:
            V.flow_mix_den(V.Timeline(step))
        assert "the denominator %d, more than 65535" % step.denominator in str(e.value) and str(step) in str(e.value)
    assert V.flow_mix_den(V.Timeline(Fr(1, 65535))) == 65535
    # through the class: the refusal comes with the timeline, before a writer is opened or a frame read
    vi = api(flow_check=True, flow_blocks=3, flow_fallback="mix", speed="333333/1000000")
    with pytest.raises(ValueError, match="the denominator 1000000, more than 65535"):
        vi.timeline((25, 1))
    # through run(): refused before the reader or the writer is touched - neither stand-in has anything but the rate
    class Untouched:
        def __getattr__(self, name):
            raise AssertionError("run() touched %s before the refusal" % name)
    with pytest.raises(ValueError, match="the denominator 1000000, more than 65535"):
        vi.run(types.SimpleNamespace(rate=(25, 1)), Untouched())
    assert api(flow_check=True, flow_blocks=3, speed="333333/1000000").timeline((25, 1)).step == Fr(333333, 1000000), "nearer takes it"
    assert api(flow_check=True, flow_blocks=3, flow_fallback="mix", target_rate=(60000, 1001)).timeline((24, 1)).step == Fr(1001, 2500)


# ---- the option's refusals -------------------------------------------------------------------------------------------------------------------
def api(**kw):
    return V.VideoInterpolator(C._Model(), C._cfg(), **kw)


def test_the_option_is_no_row_of_the_table():
    for name in ("flow_fallback", "flow_mix"):
        assert name not in V.OPTIONS and name not in V.OPTION_RULES and name not in V.FLAG_ORDER


def test_parse_flow_fallback():
    assert [V.parse_flow_fallback(x) for x in ("nearer", "mix", " MIX ", "Nearer")] == ["nearer", "mix", "mix", "nearer"]
    for bad in ("blend", "", None, 1, True, ("mix",)):
        with pytest.raises(ValueError) as e:
            V.parse_flow_fallback(bad, "--flow_fallback")
        assert str(e.value).startswith("--flow_fallback, what a failed block") and str(e.value).endswith("(got %r)" % (bad,))


def test_video_interpolator_refuses():
    with pytest.raises(ValueError) as e:
        api(flow_fallback="mix")
    assert str(e.value) == "flow_fallback=\"mix\" is what a failed block of flow_blocks carries: give flow_blocks, or leave it out"
    with pytest.raises(ValueError) as e:
        api(flow_check=True, flow_fallback="mix")
    assert str(e.value).startswith("flow_fallback=\"mix\" is what a failed block of flow_blocks carries")
    with pytest.raises(ValueError, match=r"^flow_fallback, what a failed block .* \(got 'blend'\)$"):
        api(flow_check=True, flow_blocks=3, flow_fallback="blend")
    assert api().flow_fallback == "nearer" and api(flow_fallback="nearer").flow_fallback == "nearer"
    vi = api(flow_check="1/2", flow_blocks=5, flow_fallback="mix", static=0, scene_cut="1/10")
    assert vi.flow_fallback == "mix" and vi.flow_blocks == 5 and vi.flow_repaired == []
    # what flow_blocks refuses stays refused, and the table still speaks first
    with pytest.raises(ValueError, match="^flow_blocks together with active is not available"):
        api(flow_check=True, flow_blocks=3, flow_fallback="mix", active="auto")
    with pytest.raises(ValueError) as e:
        api(flow_check=True, flow_blocks=3, flow_fallback="mix", tile=(64, 64))
    assert str(e.value) == C.api_outcome(V, ("flow_check", "tile"))[1]
    with pytest.raises(ValueError, match="^flow_blocks is the flow check's per-block fallback"):
        api(flow_blocks=3, flow_fallback="mix")


def test_the_tool_refuses():
    assert R.tool_refusal(["--flow_fallback", "mix"]) == "--flow_fallback mix is what a failed block of --flow_blocks carries: it needs --flow_blocks"
    assert R.tool_refusal(["--flow_check", "--flow_fallback", "mix"]).startswith("--flow_fallback mix is what a failed block of --flow_blocks")
    text = R.tool_refusal(["--flow_check", "--flow_blocks", "3", "--flow_fallback", "blend"])
    assert text.startswith("argument --flow_fallback: --flow_fallback, what a failed block") and text.endswith("(got 'blend')"), text
    args = R.tool_refusal(["--flow_check", "--flow_blocks", "12", "--flow_fallback", "mix"])
    assert args["flow_blocks"] == 12 and args["flow_fallback"] == "mix"
    assert R.tool_refusal(["--flow_check", "--flow_blocks", "12"])["flow_fallback"] == "nearer" == R.tool_refusal([])["flow_fallback"]
    assert R.tool_refusal(["--flow_fallback", "nearer"])["flow_fallback"] == "nearer"
    # the table has spoken first, then --flow_blocks' own refusals
    assert R.tool_refusal(["--flow_check", "--flow_blocks", "3", "--flow_fallback", "mix", "--tile", "64x64"]) == C.flag_outcome(
        __import__("interpolate_video"), ("flow_check", "tile"))
    assert R.tool_refusal(["--flow_blocks", "3", "--flow_fallback", "mix"]) == "--flow_blocks is --flow_check's per-block fallback: it needs --flow_check"


def test_the_log_lines_name_the_fallback():
    import interpolate_video as tool
    rows = [(0, 24, 96), (1, 96, 96), (2, 0, 96)]
    assert tool.flow_blocks_lines(rows, 5, "nearer") == tool.flow_blocks_lines(rows, 5)
    lines = tool.flow_blocks_lines(rows, 5, "mix")
    assert lines == ["flow blocks: K = 5, fallback mix, 3 pairs, 120 of 288 blocks replaced (41.67%), per pair at most 100.00% and at least 0.00%",
                     "flow blocks: every block failed between input frames 1 and 2"]
    assert tool.flow_blocks_lines([], 5, "mix") == ["flow blocks: K = 5, fallback mix, no pair got a synthesised frame"]


# ---- PairOptions ---------------------------------------------------------------------------------------------------------------------------
class _Sink:
    def copy_(self, *args, **kw):
        pass


def _options(**kw):
    clip = types.SimpleNamespace(h=64, w=96, fb=9216, window=None, siting=V.CENTRED, bits=8)
    opt = V.PairOptions(None, clip, flow_check=(None, 0.01, 0.5), flow_blocks=5, **kw)
    opt.dev_in, opt.lefts, opt.rights = [np.zeros((3, 4))], [0, 1], [1, 2]
    opt.dev_mask, opt.dev_failed, opt.host_failed = [np.zeros((2, 1))], [np.zeros(2)], [_Sink()]
    return opt


def test_nearer_leaves_pair_options_as_they_are(monkeypatch):
    calls = []
    monkeypatch.setattr(V, "flow_paste", lambda *a, **kw: calls.append(("paste", a[-2:])))
    monkeypatch.setattr(V, "flow_mix", lambda *a, **kw: calls.append(("mix", a[-4:])))
    plain, nearer, mix = _options(), _options(flow_fallback="nearer"), _options(flow_fallback="mix")
    assert not plain.flow_mix and not nearer.flow_mix and mix.flow_mix
    keys = lambda o: {k: v for k, v in vars(o).items() if isinstance(v, (int, bool, tuple, type(None)))}  # noqa: E731
    assert keys(plain) == keys(nearer) and keys(mix) == dict(keys(plain), flow_mix=True), "nothing more is held with mix, nothing at all with nearer"
    for opt in (plain, nearer):
        opt.paste_flow(0, 0, [(0, 2, "out", 1)])
    mix.paste_flow(0, 0, [(0, 2, "out", (1, 1, 3))])
    assert calls == [("paste", (5, 1)), ("paste", (5, 1)), ("mix", (5, 1, 1, 3))]
    with pytest.raises(AssertionError, match="flow_fallback is flow_blocks'"):
        V.PairOptions(None, types.SimpleNamespace(h=64, w=96, fb=9216, window=None), flow_check=(None, 0.01, 0.5), flow_fallback="mix")


# ---- the entry's refusals, through the library -------------------------------------------------------------------------------------------
def entry_cases():
    """(what is broken, the arguments, the message): one valid set at 16 x 24, 4:2:0, bytes, N = 2, T = 3 on made-up addresses, one
    thing broken per case; where two things are broken the earlier one of the header's order speaks.  From H and W on the rows are those
    of ssm_flow_paste_fwd (test_flow_repair_cpu), under this entry's name."""
    fb = V.frame_bytes(16, 24, V.CENTRED, 8)
    ok = dict(a=0x10000, b=0x20000, sa=fb, sb=fb, out=0x40000, so=fb, N=2, T=3, num0=1, num_step=1, den=4, H=16, W=24, layout=0, sbytes=1,
              mask=0x80000, sm=2 * 16 * 24, K=8, counts=0x90000)
    k_text = "flow_mix: k = %d + j * %d leaves 0..den=%d within T=3 outputs"
    rows = [
        ("null a", dict(a=None), "flow_mix: null pointer"),
        ("null mask and N = 0", dict(mask=None, N=0), "flow_mix: null pointer"),
        ("null counts", dict(counts=None), "flow_mix: null pointer"),
        ("N = 0 and T = 0", dict(N=0, T=0), "flow_mix: N=0 outside 1..65535"),
        ("N = 65536", dict(N=65536), "flow_mix: N=65536 outside 1..65535"),
        ("T = 65536 and den = 1", dict(T=65536, den=1), "flow_mix: T=65536 outside 1..65535"),
        ("T = 0", dict(T=0), "flow_mix: T=0 outside 1..65535"),
        ("den = 1", dict(den=1), "flow_mix: den=1 outside 2..65535"),
        ("den = 65536 and num0 = -1", dict(den=65536, num0=-1), "flow_mix: den=65536 outside 2..65535"),
        ("den = 0 and H = 0", dict(den=0, H=0), "flow_mix: den=0 outside 2..65535"),
        ("num0 = -1", dict(num0=-1), k_text % (-1, 1, 4)),
        ("num0 = 5", dict(num0=5, num_step=-1), k_text % (5, -1, 4)),
        ("the last k above den", dict(num0=1, num_step=2), k_text % (1, 2, 4)),
        ("the last k below 0", dict(num0=1, num_step=-1), k_text % (1, -1, 4)),
        ("the last k above den and H = 0", dict(num0=4, num_step=1, H=0), k_text % (4, 1, 4)),
        ("a step that would wrap 32 bits", dict(num0=0, num_step=2147483647), k_text % (0, 2147483647, 4)),
        ("H = 0 and layout = 4", dict(H=0, layout=4), "flow_mix: bad frame size 0x24"),
        ("layout = 4 and sample_bytes = 3", dict(layout=4, sbytes=3), "flow_mix: layout 4 not in {0, 1, 2, 3}"),
        ("sample_bytes = 3 and K = 65", dict(sbytes=3, K=65), "flow_mix: sample_bytes 3 not in {1, 2}"),
        ("K = 65 and a short stride of a", dict(K=65, sa=fb - 1), "flow_mix: K=65 outside 0..64"),
        ("K = -1", dict(K=-1), "flow_mix: K=-1 outside 0..64"),
        ("a short stride of b", dict(sb=1 - fb), "flow_mix: strides %d (a), %d (b) shorter than the frame's %d bytes" % (fb, 1 - fb, fb)),
        ("short strides of a and out", dict(sa=0, so=0), "flow_mix: strides 0 (a), %d (b) shorter than the frame's %d bytes" % (fb, fb)),
        ("short strides of out and mask", dict(so=fb - 1, sm=5), "flow_mix: stride %d (out) shorter than the frame's %d bytes" % (fb - 1, fb)),
        ("a short stride of mask, words at an odd address", dict(sm=767, sbytes=2, a=0x10001, sa=2 * fb, sb=2 * fb, so=2 * fb),
         "flow_mix: stride 767 (mask) shorter than a pair's two planes, 768 bytes"),
        ("words at an odd address", dict(sbytes=2, a=0x10001, sa=2 * fb + 1, sb=2 * fb, so=2 * fb),
         "flow_mix: a payload of 2-byte samples (a, b or out) is not 2-byte aligned"),
        ("words at an odd stride", dict(sbytes=2, sa=2 * fb + 1, sb=2 * fb, so=2 * fb, out=0x20000),
         "flow_mix: strides %d (a), %d (b), %d (out) of 2-byte samples must be even" % (2 * fb + 1, 2 * fb, 2 * fb)),
        ("out overlaps a", dict(out=0x10000 + fb), "flow_mix: out overlaps a, b or mask"),
        ("out overlaps b from below", dict(out=0x20000 - 6 * fb + 1), "flow_mix: out overlaps a, b or mask"),
        ("out overlaps mask, counts off", dict(out=0x80000, counts=0x90004), "flow_mix: out overlaps a, b or mask"),
        ("counts off their alignment", dict(counts=0x90004), "flow_mix: counts is not 8-byte aligned"),
    ]
    return ok, rows


def call_entry(args):
    from ssm_amd import hipbind as hb
    lib = hb.load()
    rc = lib.ssm_flow_mix_fwd(args["a"], args["b"], args["sa"], args["sb"], args["out"], args["so"], args["N"], args["T"], args["num0"],
                              args["num_step"], args["den"], args["H"], args["W"], args["layout"], args["sbytes"], args["mask"], args["sm"],
                              args["K"], args["counts"], None)
    return rc, lib.ssm_last_error_string().decode()


_OK, _ROWS = entry_cases()


@R.no_gpu
@pytest.mark.parametrize("name,broken,message", _ROWS, ids=[r[0].replace(" ", "_") for r in _ROWS])
def test_the_entry_refuses_in_order(name, broken, message):
    """Made-up addresses: every case is refused before anything is queued, and the module never sends the valid set itself."""
    assert broken, "a row breaks something"
    assert call_entry(dict(_OK, **broken)) == (-1, message)


@R.no_gpu
def test_the_entry_refuses_a_frame_of_too_many_strips():
    """2^23 x 2^20 blocks are 2^35 strips; nothing of that size is allocated, the addresses are made up."""
    big = dict(_OK, N=1, T=1, num0=1, num_step=0, den=2, a=1 << 50, b=1 << 51, out=1 << 52, mask=1 << 53)
    big.update(H=8 * (1 << 23), W=8 * (1 << 20))
    rc, text = call_entry(big)
    assert rc == -1 and text.startswith("flow_mix: a frame of ") and text.endswith("bytes is more than the grid takes")
