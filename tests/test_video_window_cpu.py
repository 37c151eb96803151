"""No-GPU checks of the shutter windows (ssm_amd.video.shutter_window, parse_shutter_window, the weights= of accumulate_host,
accumulate_light_host and accumulate_hdr_host, VideoInterpolator(shutter_window=), scripts/interpolate_video.py --shutter_window), and
the derivation of the bounds that tests/test_hip_shutter_window.py holds ssm_frames_accumulate_light_weighted_fwd and
ssm_frames_accumulate_hdr_weighted_fwd to against the float64 yardsticks.  The coded form has no bound: it is held bit for bit.

What a weighted call computes (include/ssm_hip.h): p_n = w_n * dec(src[n]);  s = init ? p_0 : acc + p_0;  s = s + p_n;  r = s * scale;
acc = enc(r) - every multiply and add one rounded fp32 operation.  The weights w_n are fp32 values that both sides read as they are (the
yardstick takes float64(w_n)), and so is the scale: neither carries an error of its own.  An output's weights are w_0 .. w_(S-1) >= 0 with
scale = fp32(1 / W), W = sum of the w_j: after normalisation a_j = w_j scale they lie in [0, 1] and are convex, sum a_j = W fp32(1 / W)
within u = 2^-24 of 1.  Against the unweighted derivations (tests/test_video_light_cpu.py, tests/test_video_hdr_cpu.py; their notation,
their assumptions: S <= 8 samples, a rounded operation off by u relative, the yardstick's float64 errors left out) this changes two things.

  One more rounding per sample.  p_n = w_n L_n (1 + d), |d| <= u: the decoded light L_n carries u L_n more.
    Power-law curves, in light: dL <= 15.6u + u = 16.6u.  In coded units, e = phi'(L) dL with encode's slope phi': the addition is
    u L phi'(L) <= u max(thr, (1 + a) / g) <= 0.5u (the line: slope L <= thr; the power: (1 + a) / g L^(1/g) <= (1 + a) / g = 0.44,
    0.495, 0.417 for srgb, bt709, bt1886): e <= 8.4u + 0.5u = 8.9u per decoded value.
    PQ and HLG: the mean of the samples' errors is at most hat(r) (the concave envelope of psi, Jensen - which holds for any convex
    combination, not only the uniform one) plus u r.

  Convex weights in place of 1 / S.  r = sum a_j L_j.
    The sum's own roundings.  Every partial sum is <= W r / (W scale) (the terms are >= 0), there are S - 1 additions and the closing
    product: after the scale (S - 1) u r + u r = S u r <= 8u r, what the box has; the per-sample products are counted above.
    Power-law curves, encode.  phi is increasing and concave and r >= a_j L_j, so phi'(r) <= phi'(a_j L_j) <= a_j^(1/g - 1) phi'(L_j)
    (the unweighted derivation's step with 1 / S = a_j: a line, then a power < 1 that leaves it at the line's slope).  Sample j's error
    a_j dL_j = a_j e_j / phi'(L_j) of r reaches the output as at most a_j^(1/g) e_j, all of them as e sum a_j^(1/g).  x^(1/g) is
    concave, so under sum a_j = 1 the sum is largest for the uniform weights: sum a_j^(1/g) <= S^(1 - 1/g) <= 8^(1 - 1/2.4) = 3.364.
    THE BOX IS THE WORST WINDOW: a taper moves weight to fewer samples, where encode's slope is smaller.  3.364 * 8.9u = 30.0u.
    The sum's roundings, phi'(r) 8u r <= 4u, and encode's own operations, 7.6u, are the unweighted ones.
      dc <= 30.0u + 4u + 7.6u = 41.6u <= 42u   (unweighted: 40u).
    Normalise, as there: dn <= (42u + u) / std + u |n|, and u |n| for the fp32 planes: bound_w(mean, std) below.  The config's mean and
    std: worst plane G, (43 + 1.088) u / 0.224 = 196.8u = 1.173e-5; rounded up to two digits that is the unweighted figure again,
      B_W_LIGHT = 1.2e-5   (unweighted: 187.9u = 1.120e-5, B = 1.2e-5).
    PQ and HLG, encode.  derive_w() is tests/test_video_hdr_cpu.py's derive() with dr = hat(r) + 9u r in place of hat(r) + 8u r; the
    intervals of decode and encode are that file's, unchanged.  B_W[name] are its values for the config's mean and std, rounded up;
    test_the_bounds_are_the_derivations prints every figure and holds them to it.

  Without the encode (a piece that is not an output's last, or a sum read as light).  sum_bound(w, held, scale, psi) below, for a call
    over weights w into an accumulator that holds a value in [0, held] (exact: both sides are given the same fp32 start), L_n in [0, 1]:
      |d acc| <= |scale| (sum w_n (psi + u) + u sum of the partial sums' bounds) + u |scale| (held + sum w_n)
    - the decode error psi and the product's u per sample, an addition's u on a partial sum that is at most held + w_0 + .. + w_n (N - 1
    additions, and the one onto the accumulator without init), the closing product.  psi = 15.6u for the power-law curves, the
    derivation's max psi for PQ and HLG.  For ones, held = 0 and N = 8 it is 8 psi + 8u + 35u + 8u: B_LIGHT of the unweighted files
    plus the eight products.

The float32 evaluation of the yardsticks is held to the same bounds here, on values that include 0, 1, the curves' thresholds with
their neighbours and out-of-range values; the kernels are held to them on the GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_video_hdr_cpu as hdr_cpu  # noqa: E402
import test_video_light_cpu as light_cpu  # noqa: E402
from ssm_amd import video as V  # noqa: E402
from ssm_amd.weights import IMAGENET_MEAN, IMAGENET_STD  # noqa: E402

U = 2.0 ** -24
MEAN, STD = IMAGENET_MEAN, IMAGENET_STD
CURVES, NAMES = light_cpu.CURVES, hdr_cpu.NAMES
WINDOWS = ("triangle", "hann", "gauss", "gauss:3/2", "gauss:0.5")
PSI_LIGHT = 15.6 * U          # tests/test_video_light_cpu.py: dL of one decoded value on either piece


# ---- the derivation ------------------------------------------------------------------------------------------------------------------
def bound_w(mean, std):
    """Power-law curves, encode = 1, convex weights over at most 8 samples, in normalised units (the docstring's 42u + u, then u |n| twice)."""
    return max((43.0 + 2.0 * max(m, 1.0 - m)) * U / s for m, s in zip(mean, std))


def sum_bound(w, held, scale, psi, init=None):
    """Without the encode: a call over the weights w into an accumulator holding a value in [0, held] (init: held == 0 by default)."""
    w = np.asarray(w, np.float64)
    init = held == 0 if init is None else init
    partial = held + np.cumsum(w)          # bounds of the partial sums after sample 0, 1, ...
    adds = partial[1:].sum() + (0.0 if init else partial[0])
    return abs(float(scale)) * (w.sum() * (psi + U) + U * adds) + U * abs(float(scale)) * (held + w.sum())


def derive_w(name):
    """tests/test_video_hdr_cpu.py derive() with one more rounding per sample: (max psi, dc of the coded weighted mean of at most 8 samples)."""
    c = hdr_cpu.codes()
    lum = V.hdr_decode_host(c, name)
    d_lo, d_hi = hdr_cpu.decode_interval(name, c)
    psi = np.maximum(d_hi - lum, lum - d_lo)
    order = np.argsort(lum, kind="stable")
    r, hat = lum[order], hdr_cpu.envelope(lum[order], np.maximum.accumulate(psi[order]))
    dr = hat + 9 * U * r
    e_lo, e_hi = hdr_cpu.encode_interval(name, r - dr, r + dr)
    back = V.hdr_encode_host(r, name)
    return float(psi.max()), float(np.maximum(e_hi - back, back - e_lo).max())


@pytest.fixture(scope="module")
def derived():
    return {name: derive_w(name) for name in NAMES}


# the derivations' values for the config's mean and std, rounded up (test_the_bounds_are_the_derivations holds them to it)
B_W_LIGHT = 1.2e-5
B_W = {"pq": 2.2e-4, "hlg": 3.5e-6}          # unweighted: 2.2e-4 (2.119e-4 either way) and 3.4e-6 (3.40e-6; weighted 3.43e-6)
PSI = {"pq": 2274.5 * U, "hlg": 26.3 * U}          # max psi of the derivation, rounded up: what sum_bound takes for the HDR lights


def test_the_bounds_are_the_derivations(derived):
    b = bound_w(MEAN, STD)
    print("power-law curves: bound_w = %.1f u = %.4g (unweighted %.1f u = %.4g); B_W = %.3g" % (b / U, b, light_cpu.bound(MEAN, STD) / U,
                                                                                                 light_cpu.bound(MEAN, STD), B_W_LIGHT))
    assert light_cpu.bound(MEAN, STD) < b <= B_W_LIGHT < 1.1 * b
    assert 8 ** (1 - 1 / 2.4) * 8.9 <= 30.0 and 30.0 + 4 + 7.6 <= 42
    for thr, slope, a, g in V.LIGHT_CURVES.values():
        assert max(thr, (1 + a) / g) <= 0.5 and g <= 2.4, "u L phi'(L) <= 0.5u and S^(1 - 1/g) <= 8^(1 - 1/2.4)"
    ones = sum_bound(np.ones(8), 0.0, 1.0, PSI_LIGHT)
    assert abs(ones - (8 * PSI_LIGHT + 8 * U + 35 * U + 8 * U)) < 1e-3 * U and ones <= light_cpu.B_LIGHT + 8 * U, \
        "ones: the unweighted B_LIGHT (170u, rounded up from 167.8u) and the eight products"
    for name, (psi, dc) in derived.items():
        bw = hdr_cpu.bound_from(dc, MEAN, STD)
        print("%s: psi <= %.1f u, weighted dc <= %.1f u = %.4g; B_W %.4g (unweighted B %.3g)" % (name, psi / U, dc / U, dc, bw, hdr_cpu.B[name]))
        assert bw <= B_W[name] < 1.1 * bw and psi <= PSI[name] < 1.01 * psi


def test_sum_of_concave_powers_is_largest_for_the_box():
    """sum a_j^(1/g) over the normalised weights of every window at S <= 8 stays at or below the box's S^(1 - 1/g)."""
    for g in (2.4, 1 / 0.45):
        for S in range(1, 9):
            for name in WINDOWS + ("box",):
                w, scale = V.shutter_window(name, S)
                a = w.astype(np.float64) * float(scale)
                assert abs(a.sum() - 1.0) <= U and a.min() >= 0 and a.max() <= 1.0
                assert (a ** (1 / g)).sum() <= S ** (1 - 1 / g) * (1 + 1e-7), (name, S)


# ---- the windows ---------------------------------------------------------------------------------------------------------------------
def test_exact_triangles():
    w, scale = V.shutter_window("triangle", 4)
    assert w.dtype == np.float32 and w.tolist() == [1, 3, 3, 1] and type(scale) is np.float32 and scale == np.float32(1 / 8)
    w, scale = V.shutter_window("triangle", 5)
    assert w.tolist() == [1, 3, 5, 3, 1] and scale.tobytes() == np.float32(1 / 13).tobytes()
    w, scale = V.shutter_window("triangle", 2)
    assert w.tolist() == [1, 1] and scale == np.float32(0.5)


@pytest.mark.parametrize("name", WINDOWS + ("box",))
@pytest.mark.parametrize("S", list(range(1, 10)) + [64])
def test_windows_are_symmetric_positive_and_normalised(name, S):
    w, scale = V.shutter_window(name, S)
    assert w.dtype == np.float32 and w.shape == (S,) and type(scale) is np.float32
    assert np.array_equal(w, w[::-1]) and np.all(w > 0) and np.all(np.isfinite(w))
    assert scale.tobytes() == np.float32(1.0 / w.astype(np.float64).sum()).tobytes(), "one float64 sum of the fp32 weights, one division, one rounding"
    u = (np.arange(S, dtype=np.float64) + 0.5) / S
    kind, k = V.parse_shutter_window(name)
    want = {"box": np.ones(S), "triangle": np.minimum(2 * np.arange(S) + 1, 2 * (S - np.arange(S)) - 1).astype(np.float64),
            "hann": np.sin(np.pi * u) ** 2, "gauss": np.exp(-0.5 * (float(k or 0) * (2 * u - 1)) ** 2)}[kind]
    assert np.array_equal(w, want.astype(np.float32))
    if kind == "triangle":
        assert np.allclose(w / w.max(), (1 - np.abs(2 * u - 1)) / (1 - np.abs(2 * u - 1)).max(), rtol=1e-6), "proportional to 1 - |2u - 1|"
    if S == 1:
        assert w.tolist() == [1.0] and scale == 1.0
    if S > 2 and kind != "box":
        assert w[0] < w[S // 2], "it falls off towards the ends"


def test_parser():
    assert V.parse_shutter_window("box") == ("box", None) and V.parse_shutter_window("hann") == ("hann", None)
    assert V.parse_shutter_window("gauss") == ("gauss", 2) == V.parse_shutter_window("gauss:2") == V.parse_shutter_window(("gauss", 2))
    assert V.parse_shutter_window("gauss:2.5") == ("gauss", V.Fraction(5, 2)) == V.parse_shutter_window(" gauss:5/2 ")
    assert [V.window_name(x) for x in ("box", "gauss", "gauss:2.5", ("hann", None))] == ["box", "gauss:2", "gauss:5/2", "hann"]
    for bad in ("boxy", "Hann", "", "triangle:2", "gauss:0", "gauss:-1", "gauss:x", "gauss:", "gauss:1/0", None, 3):
        with pytest.raises(ValueError, match=repr(bad).replace("(", r"\(")):
            V.parse_shutter_window(bad)
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="at least 1 sample"):
            V.shutter_window("hann", bad)


# ---- the coded yardstick -------------------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def mixed(rng, shape):
    """Both signs, magnitudes spread over 1e-3 .. 1e3 (tests/test_hip_shutter.py)."""
    return (rng.choice([-1.0, 1.0], shape) * 10.0 ** rng.uniform(-3, 3, shape)).astype(np.float32)


def test_ones_are_the_unweighted_sum_and_none_is_todays():
    rng = np.random.default_rng(11)
    for n in (1, 2, 7):
        for init in (0, 1):
            for scale in (1.0, np.float32(1 / 3), 0.125):
                x, start = mixed(rng, (n, 3, 5, 7)), mixed(rng, (1, 3, 5, 7))
                plain = V.accumulate_host(x, start.copy(), init, scale)
                assert np.array_equal(bits(V.accumulate_host(x, start.copy(), init, scale, weights=np.ones(n, np.float32))), bits(plain))
                assert np.array_equal(bits(V.accumulate_host(x, start.copy(), init, scale, weights=None)), bits(plain))
                s = x[0].copy() if init else start[0] + x[0]          # today's arithmetic, spelled out
                for f in x[1:]:
                    s = s + f
                assert np.array_equal(bits(plain[0]), bits(s * np.float32(scale)))


def test_the_weighted_sum_is_the_definition_in_float32():
    rng = np.random.default_rng(5)
    x, start = mixed(rng, (5, 2, 3, 4)), mixed(rng, (2, 3, 4))
    w, scale = V.shutter_window("hann", 5)
    for init in (0, 1):
        got = V.accumulate_host(x, start.copy(), init, scale, weights=w)
        want = np.empty_like(start)
        for idx in np.ndindex(start.shape):
            p = [np.float32(w[n] * x[(n,) + idx]) for n in range(5)]
            s = p[0] if init else np.float32(start[idx] + p[0])
            for n in range(1, 5):
                s = np.float32(s + p[n])
            want[idx] = np.float32(s * scale)
        assert got.dtype == np.float32 and np.array_equal(bits(got), bits(want))
    with pytest.raises(AssertionError, match="one finite weight per frame"):
        V.accumulate_host(x, start.copy(), 1, scale, weights=w[:4])
    with pytest.raises(AssertionError, match="one finite weight per frame"):
        V.accumulate_host(x, start.copy(), 1, scale, weights=[1, 1, np.nan, 1, 1])


def test_pieces_equal_the_one_call():
    rng = np.random.default_rng(7)
    x, start = mixed(rng, (7, 3, 5, 7)), mixed(rng, (1, 3, 5, 7))
    for name in WINDOWS:
        w, scale = V.shutter_window(name, 7)
        for init in (0, 1):
            one = V.accumulate_host(x, start.copy(), init, scale, weights=w)
            acc = start.copy()
            V.accumulate_host(x[:3], acc, init, 1.0, weights=w[:3])
            V.accumulate_host(x[3:], acc, 0, scale, weights=w[3:])
            assert np.array_equal(bits(acc), bits(one)), (name, init)


# ---- the yardsticks in light: float32 against float64 within the derived bounds ------------------------------------------------------------
def grid(rng, n, thresholds):
    """Normalised planes [n,3,6,16] whose coded values are random in [0, 1], with 0, 1, the thresholds and their fp32 neighbours, tiny
    values and values outside [0, 1] in the first places of every plane, in other places from frame to frame; the last pixel is black."""
    m, s = (np.asarray(x, np.float32).reshape(1, 3, 1, 1) for x in (MEAN, STD))
    c = rng.uniform(0.0, 1.0, (n, 3, 6, 16)).astype(np.float32)
    special = [0.0, 1.0, 1e-6, 1 / 1023, -0.25, 1.5, -1e-3, 1.001]
    for t in thresholds:
        t = np.float32(t)
        special += [t, np.nextafter(t, np.float32(-1)), np.nextafter(t, np.float32(2))]
    flat = c.reshape(n, 3, -1)
    for f in range(n):
        flat[f, :, :len(special)] = np.roll(np.float32(special), f)
    x = ((c - m) / s).astype(np.float32)
    x.reshape(n, 3, -1)[:, :, -1] = ((np.float32(0.0) / np.float32(255.0) - m) / s)[0, :, 0, 0]
    return x


def both(host, x, w, scale, encode, pieces, **kw):
    """(float32, float64) evaluations of a yardstick over the frames x in `pieces` consecutive calls; the last scales and, if asked, encodes."""
    out = []
    cuts = np.linspace(0, x.shape[0], pieces + 1).astype(int)
    for dt in (np.float32, np.float64):
        acc = np.full((1,) + x.shape[1:], np.nan, dt)
        for i in range(pieces):
            last = i == pieces - 1
            host(x[cuts[i]:cuts[i + 1]], acc, i == 0, scale if last else 1.0, MEAN, STD, kw["row"], last and encode, dt,
                 weights=w[cuts[i]:cuts[i + 1]])
        out.append(acc.astype(np.float64))
    return out


@pytest.mark.parametrize("window", ["triangle", "hann", "gauss"])
@pytest.mark.parametrize("S", [5, 8])
def test_float32_yardsticks_lie_within_the_bounds(window, S):
    w, scale = V.shutter_window(window, S)
    rng = np.random.default_rng(S)
    black = ((np.float32(0.0) / np.float32(255.0) - np.float32(MEAN)) / np.float32(STD)).astype(np.float32)
    for name in CURVES + NAMES:
        hdr = name in NAMES
        host = V.accumulate_hdr_host if hdr else V.accumulate_light_host
        row = name if hdr else V.light_curve(name)
        x = grid(rng, S, [0.5] if hdr else [float(row[0])])
        bar, psi = (B_W[name], PSI[name]) if hdr else (B_W_LIGHT, PSI_LIGHT)
        for pieces in (1, 2):
            f32, f64 = both(host, x, w, scale, True, pieces, row=row)
            d = np.abs(f32 - f64).max()
            l32, l64 = both(host, x, w, 1.0, False, pieces, row=row)
            dl, bl = np.abs(l32 - l64).max(), sum_bound(w, 0.0, 1.0, psi)
            print("%s %s S=%d in %d piece(s): |float32 - float64| %.3g of %.3g encoded, %.3g of %.3g in light" % (name, window, S, pieces, d, bar, dl, bl))
            assert d <= bar and dl <= bl
            assert np.array_equal(f64[0].reshape(3, -1)[:, -1].astype(np.float32), black), "black stays black under any weights"
            assert np.all(l64[0].reshape(3, -1)[:, -1] == 0.0) and np.all(l32[0].reshape(3, -1)[:, -1] == 0.0)


def test_light_yardsticks_with_ones_and_none():
    """weights=None is the arithmetic as it was; ones give the same float64 bits (1.0 * x is x)."""
    rng = np.random.default_rng(3)
    x = grid(rng, 4, [0.5])
    for name in CURVES + NAMES:
        hdr = name in NAMES
        host = V.accumulate_hdr_host if hdr else V.accumulate_light_host
        row = name if hdr else V.light_curve(name)
        run = lambda **kw: host(x, np.zeros((1,) + x.shape[1:]), 1, np.float32(0.25), MEAN, STD, row, 1, **kw)
        assert np.array_equal(run(), run(weights=None)) and np.array_equal(run(), run(weights=np.ones(4, np.float32)))
        assert not np.array_equal(run(), run(weights=V.shutter_window("triangle", 4)[0]))


# ---- constructor and command line ----------------------------------------------------------------------------------------------------
class _Cfg:
    def getint(self, section, key):
        return 2


def test_constructor():
    assert V.VideoInterpolator(None, _Cfg()).shutter_window == ("box", None)
    assert V.VideoInterpolator(None, _Cfg(), target_rate=(24, 1), shutter="1/2").shutter_window == ("box", None)
    assert V.VideoInterpolator(None, _Cfg(), shutter_window="box").shutter_window == ("box", None)
    for name, want in (("triangle", ("triangle", None)), ("hann", ("hann", None)), ("gauss", ("gauss", 2)), ("gauss:3/2", ("gauss", V.Fraction(3, 2)))):
        for light in ("coded", "srgb", "pq"):
            vi = V.VideoInterpolator(None, _Cfg(), target_rate=(24, 1), shutter="1/2", shutter_window=name, shutter_light=light)
            assert vi.shutter_window == want
        with pytest.raises(ValueError, match="shutter_window=%r.*give a shutter" % name):
            V.VideoInterpolator(None, _Cfg(), target_rate=(24, 1), shutter_window=name)
    with pytest.raises(ValueError, match="'cosine'"):
        V.VideoInterpolator(None, _Cfg(), target_rate=(24, 1), shutter="1/2", shutter_window="cosine")
    with pytest.raises(ValueError, match="'gauss:0'"):
        V.VideoInterpolator(None, _Cfg(), target_rate=(24, 1), shutter="1/2", shutter_window="gauss:0")


BASE = ["-c", "x.ini", "--expt", "e", "--log", "l", "--input", "-", "--output", "-"]


def test_cli_flag():
    import interpolate_video as cli
    assert cli.getargs(BASE).shutter_window == ("box", None)
    assert cli.getargs(BASE + ["--fps", "24", "--shutter", "180"]).shutter_window == ("box", None)
    for text, want in (("box", ("box", None)), ("triangle", ("triangle", None)), ("hann", ("hann", None)), ("gauss", ("gauss", 2)),
                       ("gauss:2.5", ("gauss", V.Fraction(5, 2)))):
        a = cli.getargs(BASE + ["--fps", "24", "--shutter", "180", "--shutter_light", "srgb", "--shutter_window", text])
        assert a.shutter_window == want
    assert cli.getargs(BASE + ["--fps", "24", "--shutter_window", "box"]).shutter_window == ("box", None), "the default, given: nothing to refuse"


@pytest.mark.parametrize("extra,named", [(["--fps", "24", "--shutter", "180", "--shutter_window", "cosine"], "'cosine'"),
                                         (["--fps", "24", "--shutter", "180", "--shutter_window", "gauss:0"], "'gauss:0'"),
                                         (["--fps", "24", "--shutter", "180", "--shutter_window", "gauss:-1"], "'gauss:-1'"),
                                         (["--fps", "24", "--shutter", "180", "--shutter_window", "gauss:x"], "'gauss:x'"),
                                         (["--fps", "24", "--shutter_window", "hann"], "--shutter_window hann is the window of the sub-frames that --shutter averages"),
                                         (["--shutter_window", "gauss:3"], "--shutter_window gauss:3 is the window of the sub-frames that --shutter averages")])
def test_cli_errors(capsys, extra, named):
    import interpolate_video as cli
    with pytest.raises(SystemExit) as e:
        cli.getargs(BASE + extra)
    assert e.value.code == 2
    assert named in capsys.readouterr().err
