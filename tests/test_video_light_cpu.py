"""No-GPU checks of the shutter in linear light (ssm_amd.video.light_curve, accumulate_light_host, VideoInterpolator(shutter_light=),
scripts/interpolate_video.py --shutter_light), and the derivation of the bound B that tests/test_hip_shutter_light.py holds
ssm_frames_accumulate_light_fwd to against the float64 yardstick.

The curves.  bt709's row is not the standard's three printed digits (0.018, 1.099): with them the two pieces of the curve miss each
other at the join by 5.5e-5 of L and 2.5e-4 of c, which test_branches_agree_at_the_join would report.  The row holds the solution of
the two conditions those digits were rounded from (the pieces meet in value and in slope), which test_bt709_constants checks.  The
round trip "S copies of a frame give it back" holds to 1e-12 because the float64 yardstick keeps the row's fp32 thr, slope, a and g and
takes their reciprocals in float64 (light_decode_host / light_encode_host say why); a c within ~3e-8 above thr is the one exception,
since there the pieces' remaining mismatch lets encode take the other piece: random values do not fall there and the test names the window.

Bound of the kernel, |kernel - float64 yardstick| in normalised units, S <= 8 samples, scale = fp32(1 / S).  u = 2^-24: a rounded fp32
operation is off by u relative at most; v_log_f32 and v_exp_f32 are 1 ulp instructions (ISA manual), 2u relative.  The yardstick's
float64 errors (1e-16) are left out.  The constants the kernel multiplies by - 1/slope, 1/(1+a), 1/g, thr/slope, 1+a - are float64
values rounded once, each u relative off the float64 reciprocal of the row's primary constant that the yardstick uses; the terms
marked (k) carry them.
  Decode.  c = clip(v std + mean): two operations on magnitudes <= 1 wherever the clip does not absorb them, |dc| <= 2u.
    Linear piece, L = c (1/slope): dL <= (1/slope) dc + 2u L (product, (k)).  In coded units e = slope dL <= 2u + 2u thr <= 2.2u.
    Power piece, x = (c + a)(1/(1+a)) <= 1: the sum carries dc + 1.1u, the product u x and (k) u x: dx <= 3.1u + 2u = 5.1u.
      l = log2 x: dl <= dx / (x ln 2) + 2u |l|;  q = g l: dq <= g dl + u |q|;  L = 2^q: dL <= L ln 2 dq + 2u L, so
      dL <= L (g dx / x + 3u ln 2 |q| + 2u).  In coded units, with encode's slope phi'(L) = (1+a)(1/g) L^(1/g - 1) and L^(1/g) = x:
      e = phi'(L) dL <= (1+a)(dx + x 3u ln 2 |log2 x| + 2u x / g) <= 1.1 (5.1u + 3u ln 2 * 0.531 + 2u * 0.45) = 7.9u,
      0.531 = max of x |log2 x|.  In light itself (x <= 1, L <= 1, L |q| <= 0.531): dL <= 2.4 * 5.1u + 1.2u + 2u <= 15.5u.
    A c that the two sides put on different pieces adds the pieces' mismatch there: <= 4.2e-9 of L, <= 3e-8 = 0.5u of c (test below).
    So e <= 8.4u per decoded value on either piece; dL <= 15.6u.
  Sum of S values in [0, 1] and the scale: every partial sum is <= S r (r the mean), S - 1 additions and one product:
    dr <= (sum of the dL_i) / S + 8u r.  With encode = 0 and any |scale| <= 1, at most 8 values: |d acc| <= 8 * 15.6u + 35u + 8u < 170u
    = B_LIGHT (35 = 2 + 3 + ... + 8, partial sums <= their count).
  Encode.  phi is increasing and concave (a line, then a power < 1 that leaves it at the line's slope), and r >= L_i / S for every
    sample, so phi'(r) <= phi'(L_i / S) <= S^(1 - 1/g) phi'(L_i): a decode error of e_i coded units reaches the output as at most
    S^(-1/g) e_i, all S of them as S^(1 - 1/g) 8.4u <= 8^(1 - 1/2.4) 8.4u = 28.3u (S = 8, bt1886 and srgb).  This holds down to black:
    bt1886's encode has no bounded slope at 0, and needs none.
    The sum's roundings: phi'(r) 8u r <= 8u max(thr, (1+a)/g) <= 4u.
    Its own operations: line, c = r slope: u c <= 0.1u.  Power, p = r^(1/g) by the same three instructions: dp <= p (3u ln 2 |log2 p|
    + 2u), times 1+a: 1.1 (1.11u + 2u) = 3.4u; (k) the exponent's rounding moves p by u ln 2 p |log2 p|: 1.1 * 0.37u = 0.4u; the product
    (1+a) p, u and (k) u: 2.2u; the difference u |c| <= u: 7.1u in all.  The other piece at the join: 0.5u.  Encode <= 7.6u.
    dc <= 28.3u + 4u + 7.6u = 39.9u <= 40u.
  Normalise, n = (c - mean) / std: the difference u |c - mean| <= u, the quotient u |n|: dn <= 41u / std + u |n|, |n| <= max(mean,
    1 - mean) / std.  The config's mean (0.485, 0.456, 0.406) and std (0.229, 0.224, 0.225): worst plane G, 41u / 0.224 + 2.43u =
    185.5u = 1.11e-5; rounding the float64 accumulator to the fp32 planes the egress reads adds u |n| <= 2.7u.
  B = bound(config) = 1.2e-5 (bound() below, rounded up); 1/4 of an 8-bit code step at the largest 1/std is (1/255) / 0.224 / 4 = 4.4e-3,
  370 times that.  tools/bench_shutter_light.py prints the worst distance it sees on random frames (profiles/shutter_light_bench.txt)."""
import numpy as np
import pytest

from ssm_amd import video as V
from ssm_amd.weights import IMAGENET_MEAN, IMAGENET_STD

U = 2.0 ** -24
B_LIGHT = 170 * U          # encode = 0: sums of at most 8 samples, |scale| <= 1
CURVES = ("bt709", "srgb", "bt1886")


def bound(mean, std):
    """The bound of the docstring for encode = 1, scale = 1 / (samples summed), at most 8 of them, in normalised units."""
    return max((41.0 + 2.0 * max(m, 1.0 - m)) * U / s for m, s in zip(mean, std))


B = 1.2e-5
MEAN, STD = IMAGENET_MEAN, IMAGENET_STD


def test_the_bound_is_the_docstrings():
    assert bound(MEAN, STD) <= B < 1.1 * bound(MEAN, STD)
    assert B * 255 * max(STD) < 1e-3 and B < (1 / 255) / min(STD) / 4 / 100, "far inside a quarter of a code step"


# ---- curves --------------------------------------------------------------------------------------------------------------------------
def test_rows_are_float64_constants_rounded_once():
    assert V.LIGHT_ROW == 9 and set(V.LIGHT_CURVES) == set(CURVES) and V.SHUTTER_LIGHTS == ("coded",) + tuple(V.LIGHT_CURVES)
    want = {"srgb": (0.04045, 12.92, 0.055, 2.4), "bt1886": (0.0, 1.0, 0.0, 2.4),
            "bt709": (4.5 * 0.018053968510807, 4.5, 1.09929682680944 - 1.0, 1.0 / 0.45)}
    for name, (thr, slope, a, g) in want.items():
        row = V.light_curve(name)
        assert row.dtype == np.float32 and row.shape == (9,)
        exp = [np.float32(x) for x in (thr, 1.0 / slope, a, 1.0 / (1.0 + a), g, thr / slope, slope, 1.0 + a, 1.0 / g)]
        assert [x.tobytes() for x in row] == [x.tobytes() for x in exp], name
    with pytest.raises(ValueError, match="'coded'"):
        V.light_curve("coded")          # today's behaviour has no row
    with pytest.raises(ValueError, match="'pq'"):
        V.light_curve("pq")


def test_bt709_constants():
    """thr = 4.5 beta and a = alpha - 1 with (alpha, beta) where V = 4.5 L and V = alpha L^0.45 - (alpha - 1) meet in value and slope; to
    three digits they are the standard's 0.018 and 1.099 (0.081 and 0.099 of the curve table)."""
    thr, slope, a, g = V.LIGHT_CURVES["bt709"]
    beta, alpha = thr / slope, 1.0 + a
    assert abs(4.5 * beta - (alpha * beta ** 0.45 - (alpha - 1.0))) < 1e-14 and abs(4.5 - 0.45 * alpha * beta ** -0.55) < 1e-11
    assert round(beta, 3) == 0.018 and round(alpha, 3) == 1.099 and round(thr, 3) == 0.081 and round(a, 3) == 0.099 and slope == 4.5


@pytest.mark.parametrize("name", CURVES)
def test_branches_agree_at_the_join(name):
    row = V.light_curve(name).astype(np.float64)
    thr, islope, a, i1a, g, lthr, slope, a1, ig = row
    lin, pw = thr * islope, ((thr + a) * i1a) ** g
    print("%s decode at thr: line %.12g power %.12g, %.3g apart" % (name, lin, pw, abs(lin - pw)))
    assert abs(lin - pw) <= 1e-6
    assert abs(lin - pw) <= 4.2e-9, "what the bound's docstring counts on"
    lin, pw = lthr * slope, a1 * lthr ** ig - a
    print("%s encode at thr / slope: line %.12g power %.12g, %.3g apart" % (name, lin, pw, abs(lin - pw)))
    assert abs(lin - pw) <= 1e-6
    assert abs(lin - pw) <= 3e-8, "what the bound's docstring counts on"
    # the yardstick's own functions take the same pieces
    below, above = np.nextafter(row[0], -1.0), np.nextafter(row[0], 2.0)
    d = V.light_decode_host(np.array([below, row[0], above]), V.light_curve(name))
    assert abs(d[1] - thr * islope) < 1e-9 and abs(d[2] - pw) < 1 and abs(d[2] - d[1]) <= 1e-6


@pytest.mark.parametrize("name", CURVES)
def test_decode_and_encode_are_inverse_and_monotone(name):
    row = V.light_curve(name)
    c = np.linspace(0.0, 1.0, 4097)
    lum = V.light_decode_host(c, row)
    assert lum[0] == 0.0 and abs(lum[-1] - 1.0) < 1e-7 and np.all(np.diff(lum) > 0)
    back = V.light_encode_host(lum, row)
    away = np.abs(c - float(row[0])) > 1e-6
    assert np.abs(back - c)[away].max() < 1e-12


# ---- the yardstick in float64 --------------------------------------------------------------------------------------------------------
def normalised(c, mean=MEAN, std=STD):
    """Coded planes [N,3,H,W] in [0, 1] -> the path's normalised fp32 planes."""
    m, s = (np.asarray(x, np.float32).reshape(1, 3, 1, 1) for x in (mean, std))
    return ((np.asarray(c, np.float32) - m) / s).astype(np.float32)


def run(frames, name, calls, scale, mean=MEAN, std=STD, dtype=np.float64):
    """The frames through accumulate_light_host in `calls` consecutive pieces; the last call scales and encodes."""
    acc = np.full((1,) + frames.shape[1:], np.nan, dtype)
    cuts = np.linspace(0, frames.shape[0], calls + 1).astype(int)
    for i in range(calls):
        last = i == calls - 1
        out = V.accumulate_light_host(frames[cuts[i]:cuts[i + 1]], acc, i == 0, scale if last else 1.0, mean, std, V.light_curve(name), last, dtype)
        assert out is acc
    return acc


@pytest.mark.parametrize("name", CURVES)
@pytest.mark.parametrize("S,calls", [(1, 1), (3, 1), (8, 1), (3, 3), (8, 3)])
def test_copies_of_one_frame_give_it_back(name, S, calls):
    """Within 1e-12 for values in [0, 1], in one call and through init / several calls.  Values within 1e-6 of thr are moved off it: just above thr the two
    pieces' mismatch (3e-8 of c) lets encode take the line where decode took the power."""
    rng = np.random.default_rng(S)
    c = rng.uniform(0.001, 0.999, (1, 3, 9, 11))          # exact 0 and 1 leave [0, 1] by the planes' own fp32 rounding and are clipped
    c[0, :, 0, :3] = (0.001, 0.999, 0.5)
    thr = float(V.light_curve(name)[0])
    c[np.abs(c - thr) < 1e-6] = thr / 2
    x = normalised(c)
    got = run(np.repeat(x, S, axis=0), name, calls, 1.0 / S)
    assert got.dtype == np.float64 and np.abs(got[0] - x[0].astype(np.float64)).max() < 1e-12


def test_black_and_white_meet_at_188_under_srgb():
    """Full-range 4:4:4 grey: the mean of code 0 and code 255 is 128 on the codes and 188 in light."""
    x = normalised(np.stack([np.zeros((3, 4, 4)), np.ones((3, 4, 4))]))
    coded = V.accumulate_host(x, np.zeros((1, 3, 4, 4), np.float32), 1, 0.5)
    light = run(x, "srgb", 1, 0.5).astype(np.float32)
    hp = np.zeros((1, 3, 32, 32), np.float32)

    def luma(acc):
        hp[:, :, 14:18, 14:18] = acc
        return V.frames_to_yuv_host(hp, 4, 4, V.C444, V.BT709, V.FULL)[0]
    assert set(luma(coded)[:16]) == {128} and set(luma(light)[:16]) == {188}
    assert set(luma(light)[16:]) == {128}, "grey has no chroma"
    assert set(luma(run(x, "bt1886", 1, 0.5).astype(np.float32))[:16]) == {191} and set(luma(run(x, "bt709", 1, 0.5).astype(np.float32))[:16]) == {180}


@pytest.mark.parametrize("name", CURVES)
def test_values_outside_count_as_0_and_1(name):
    rng = np.random.default_rng(2)
    c = rng.uniform(-0.5, 1.5, (4, 3, 5, 7))
    c[0, :, 0, 0], c[1, :, 0, 0] = -3.0, 7.0
    got = run(normalised(c), name, 2, 0.25)
    want = run(normalised(np.clip(c, 0.0, 1.0)), name, 2, 0.25)
    assert np.abs(got - want).max() < 1e-6, "fp32 planes of clipped and unclipped values differ by their own rounding only"
    assert (c < 0).any() and (c > 1).any()
    # where the coded mean lets them cancel: -0.5 and 1.5 average to 0.5 on the codes, to the mean of black and white in light
    pair = normalised(np.stack([np.full((3, 2, 2), -0.5), np.full((3, 2, 2), 1.5)]))
    bw = normalised(np.stack([np.zeros((3, 2, 2)), np.ones((3, 2, 2))]))
    assert np.abs(run(pair, name, 1, 0.5) - run(bw, name, 1, 0.5)).max() < 1e-6


@pytest.mark.parametrize("name", CURVES)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_black_stays_exactly_black(name, dtype):
    m, s = np.float32(MEAN), np.float32(STD)
    black = ((np.float32(0.0) / np.float32(255.0) - m) / s).astype(np.float32)          # the ingest kernels' pad value
    x = np.broadcast_to(black.reshape(1, 3, 1, 1), (5, 3, 4, 6)).copy()
    x[:, :, 2:, :] = normalised(np.random.default_rng(3).uniform(0, 1, (5, 3, 2, 6)))
    x[2, :, 0, 0] = -7.5          # below black: exactly no light
    got = run(x, name, 2, np.float32(1.0 / 5.0), dtype=dtype)
    want = ((dtype(0.0) - m.astype(dtype)) / s.astype(dtype)).reshape(3, 1, 1)
    assert np.array_equal(got[0, :, :2, :], np.broadcast_to(want, (3, 2, 6)))
    assert np.array_equal(got[0, :, :2, :].astype(np.float32), np.broadcast_to(black.reshape(3, 1, 1), (3, 2, 6)))
    light = V.accumulate_light_host(x, np.zeros((3, 4, 6), dtype), 1, 1.0, MEAN, STD, V.light_curve(name), 0, dtype)
    assert np.all(light[:, :2, :] == 0.0)


@pytest.mark.parametrize("name", CURVES)
def test_several_calls_equal_one(name):
    x = normalised(np.random.default_rng(4).uniform(-0.1, 1.1, (7, 3, 5, 7)))
    one = run(x, name, 1, np.float32(1.0 / 7.0))
    for calls in (2, 3, 7):
        assert np.array_equal(run(x, name, calls, np.float32(1.0 / 7.0)), one), "the same additions in the same order"


def test_float32_yardstick_lies_within_the_bound_too():
    x = normalised(np.random.default_rng(5).uniform(0.0, 1.0, (8, 3, 16, 16)))
    for name in CURVES:
        d = np.abs(run(x, name, 2, np.float32(0.125), dtype=np.float32).astype(np.float64) - run(x, name, 2, np.float32(0.125)))
        print("%s: float32 yardstick - float64 yardstick: %.3g at most (B = %.3g)" % (name, d.max(), B))
        assert d.max() < B


# ---- constructor and command line -------------------------------------------------------------------------------------------------------
class _Cfg:
    def getint(self, section, key):
        return 2


def test_constructor_refusals():
    vi = V.VideoInterpolator(None, _Cfg(), target_rate=(24, 1), shutter="1/2")
    assert vi.shutter_light == "coded"
    for name in CURVES:
        assert V.VideoInterpolator(None, _Cfg(), target_rate=(24, 1), shutter="1/2", shutter_light=name).shutter_light == name
    with pytest.raises(ValueError, match="'linear'"):
        V.VideoInterpolator(None, _Cfg(), target_rate=(24, 1), shutter="1/2", shutter_light="linear")
    with pytest.raises(ValueError, match="shutter_light='srgb'.*give a shutter"):
        V.VideoInterpolator(None, _Cfg(), target_rate=(24, 1), shutter_light="srgb")
    assert V.VideoInterpolator(None, _Cfg(), shutter_light="coded").shutter_light == "coded"


BASE = ["-c", "x.ini", "--expt", "e", "--log", "l", "--input", "-", "--output", "-"]


def test_cli_flag():
    import interpolate_video as cli
    assert cli.getargs(BASE).shutter_light == "coded"
    assert cli.getargs(BASE + ["--fps", "24", "--shutter", "180"]).shutter_light == "coded"
    for name in ("coded",) + CURVES:
        assert cli.getargs(BASE + ["--fps", "24", "--shutter", "180", "--shutter_light", name]).shutter_light == name


@pytest.mark.parametrize("extra,named", [(["--fps", "24", "--shutter", "180", "--shutter_light", "linear"], "'linear'"),
                                         (["--fps", "24", "--shutter_light", "srgb"], "--shutter_light srgb is the light in which --shutter averages"),
                                         (["--shutter_light", "bt709"], "--shutter_light bt709 is the light in which --shutter averages")])
def test_cli_errors(capsys, extra, named):
    import interpolate_video as cli
    with pytest.raises(SystemExit) as e:
        cli.getargs(BASE + extra)
    assert e.value.code == 2
    assert named in capsys.readouterr().err
