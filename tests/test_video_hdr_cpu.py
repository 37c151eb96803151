"""No-GPU checks of HDR clips in the streamed tool: the BT.2020 matrix (ssm_amd.video.BT2020, yuv_table(bits, BT2020), table_index), PQ
and HLG as the shutter's light (hdr_light, hdr_decode_host / hdr_encode_host, accumulate_hdr_host, VideoInterpolator(shutter_light=),
the two scripts' options), and the derivation of the bounds that tests/test_hip_video_hdr.py holds ssm_frames_accumulate_hdr_fwd to
against the float64 yardstick.

Bound of the kernel, |kernel - float64 yardstick|, S <= 8 samples, scale = fp32(1 / S).  u = 2^-24.  As tests/test_video_light_cpu.py:
a rounded fp32 operation is off by u relative at most; v_log_f32, v_exp_f32, v_rcp_f32 and v_sqrt_f32 are 1 ulp instructions (ISA
manual), 2u relative; a row constant that is not exact in fp32 is u relative off the float64 constant the yardstick uses (the PQ
constants c1, c2, c3, m1, m2 are dyadic and exact; 1/m1, 1/m2 and all of HLG's are rounded).  The yardstick's own float64 errors are left
out.  Where the power-law curves allow a closed form, these two do not (PQ's 1/m2 = 0.0127 and m2 = 78.8 turn a relative error of p
into 79 times that of c, and p - c1 cancels), so the bound is EVALUATED here, by interval arithmetic over a grid of codes, from those
per-operation errors and nothing else - decode_interval() and encode_interval() below follow the kernel's steps and widen [lo, hi] at every one.
Every step is monotone in its operand, so an interval's ends are the images of its operand's ends.
  Decode.  c = clip(v std + mean): |dc| <= 2u.  decode_interval(name, c) encloses what the kernel's decode gives for any c' within 2u
    of c; psi(c) = its distance from the float64 decode(c), an error in light.  B_LIGHT: with encode = 0, at most 8 values and
    |scale| <= 1, |d acc| <= 8 max psi + 35u + 8u (35 = 2 + ... + 8: partial sums are at most their count).
  Sum of S values and the scale.  r = mean of the L_i; dr <= mean of psi_i + 8u r (S - 1 additions on partial sums <= S r, one product).
    The mean of psi over samples whose light has mean r is at most hat(r), the upper concave envelope of psi as a function of L =
    decode(c) at r (Jensen) - envelope() below.
  Encode.  encode_interval(name, r_lo, r_hi) encloses the kernel's encode of any r' in [r - dr, r + dr]; its distance from the float64
    encode(r), maximised over a grid of r, is the error dc of the coded mean.  The quotient (c1 + c2 y) / (1 + c3 y) is taken at the
    ends of y's interval as ONE increasing function of y - numerator and denominator rise together, and widening them separately would
    charge c2 dy / n + c3 dy / d where the function moves by their difference - and the roundings of its four operations (7u relative)
    are added to the result.  PQ's step at L = 0 (L <= 0 takes c = 0, the formula gives c1 ^ m2 = 7.3e-7) is inside: an r whose interval
    reaches 0 may come out as 0.
  Normalise, n = (c - mean) / std: dn <= (dc + u) / std + u |n|, |n| <= max(mean, 1 - mean) / std; rounding the float64 accumulator to
    the fp32 planes the egress reads adds u |n|.
bound_from(dc, mean, std) is that, and B[name] its value for the config's mean and std, rounded up; test_the_bounds_are_the_derivations
prints every figure.  What the derivation reaches: HLG psi <= 26.2u, dc <= 10.5u, B = 3.4e-6, 310 times inside a quarter of a 10-bit
code step at the largest std.  PQ psi <= 2274u (at white the EOTF's denominator c2 - c3 p is 0.164 and carries 114 times p's relative
error, then the power 1 / m1 = 6.3), dc <= 794u = 4.7e-5 of c (m2 = 79 times the seven roundings of the closing quotient alone is 553u),
B = 2.2e-4: 19 times inside a quarter of an 8-bit step, 4.8 times inside a quarter of a 10-bit step.  The derivation cannot promise PQ
the two orders of magnitude the power-law curves have at 10 bits, and the test asserts the factor 4 it does reach (100 for HLG).
tools/bench_shutter_hdr.py prints the worst distance it sees on random frames (profiles/shutter_hdr_bench.txt)."""
import math

import numpy as np
import pytest

from ssm_amd import video as V
from ssm_amd.weights import IMAGENET_MEAN, IMAGENET_STD

U = 2.0 ** -24
MEAN, STD = IMAGENET_MEAN, IMAGENET_STD
NAMES = ("pq", "hlg")
M1, M2, C1, C2, C3 = V.PQ_M1, V.PQ_M2, V.PQ_C1, V.PQ_C2, V.PQ_C3
A, HB, CC = V.HLG_A, V.HLG_B, V.HLG_CC


# ---- the derivation ------------------------------------------------------------------------------------------------------------------
def _pow_interval(lo, hi, e, k):
    """[lo, hi] ^ e by v_log_f32, a product with e (k = 1: e is a rounded constant, 0: exact) and v_exp_f32: l = log2 x off by 2u |l|,
    q = e l by (1 + k) u |q|, 2 ^ q by ln 2 dq + 2u relative - together (3 + k) u ln 2 |log2 y| + 2u of y = x ^ e.  x = 0 gives 0."""
    def end(x, sign):
        y = np.power(x, e)
        with np.errstate(divide="ignore", invalid="ignore"):
            slack = np.where(y > 0, (3 + k) * U * math.log(2.0) * y * np.abs(np.log2(np.where(y > 0, y, 1.0))) + 2 * U * y, 0.0)
        return np.maximum(y + sign * slack, 0.0)
    return end(lo, -1), end(hi, +1)


def decode_interval(name, c):
    """Lower and upper ends of the kernel's decode over every c' in [c - 2u, c + 2u] within [0, 1]."""
    lo, hi = np.clip(c - 2 * U, 0.0, 1.0), np.clip(c + 2 * U, 0.0, 1.0)
    if name == "pq":
        p_lo, p_hi = _pow_interval(lo, hi, 1.0 / M2, 1)
        n_lo, n_hi = np.maximum(p_lo - C1, 0.0) * (1 - U), np.maximum(p_hi - C1, 0.0) * (1 + U)
        d_lo, d_hi = (C2 - C3 * p_hi * (1 + U)) * (1 - U), (C2 - C3 * p_lo * (1 - U)) * (1 + U)
        x_lo, x_hi = n_lo / d_hi * (1 - 2 * U) * (1 - U), n_hi / d_lo * (1 + 2 * U) * (1 + U)          # v_rcp_f32, then the product
        return _pow_interval(x_lo, x_hi, 1.0 / M1, 1)

    def pieces(x, s):          # both pieces at x with every rounding pushed the way of s
        sq = x * x / 3.0 * (1 + s * 3 * U)                                        # two products and the rounded 1/3
        t = (x - CC) / A
        dt = (U * abs(CC) + U * np.abs(x - CC)) / A + 2 * U * np.abs(t)           # rounded cc, the difference; the product and rounded log2(e)/a
        e = np.exp(t + s * dt) * (1 + s * 2 * U)                                   # v_exp_f32
        ex = (e + HB * (1 + s * U)) * (1 + s * U) / 12.0 * (1 + s * 2 * U)        # rounded b, the sum; the product and the rounded 1/12
        return sq, ex
    sq_lo, ex_lo = pieces(lo, -1)
    sq_hi, ex_hi = pieces(hi, +1)
    below, above = hi <= 0.5, lo > 0.5          # otherwise c' may fall on either piece
    l = np.where(below, sq_lo, np.where(above, ex_lo, np.minimum(sq_lo, ex_lo)))
    h = np.where(below, sq_hi, np.where(above, ex_hi, np.maximum(sq_hi, ex_hi)))
    return l, h


def encode_interval(name, lo, hi):
    """Lower and upper ends of the kernel's encode over every r' in [lo, hi]."""
    lo = np.maximum(lo, 0.0)
    if name == "pq":
        y_lo, y_hi = _pow_interval(lo, hi, M1, 0)
        x_lo, x_hi = (C1 + C2 * y_lo) / (1 + C3 * y_lo) * (1 - 7 * U), (C1 + C2 * y_hi) / (1 + C3 * y_hi) * (1 + 7 * U)
        c_lo, c_hi = _pow_interval(x_lo, x_hi, M2, 0)
        return np.where(lo <= 0.0, 0.0, c_lo), c_hi

    def pieces(x, s):
        sq = np.sqrt(3.0 * x * (1 + s * U)) * (1 + s * 2 * U)                      # the product, v_sqrt_f32
        w = np.maximum(12.0 * x * (1 + s * U) - HB * (1 - s * U), 1e-300) * (1 + s * U)          # the product, rounded b, the difference
        lg = np.log2(w)
        lg = lg + s * 2 * U * np.abs(lg)                                           # v_log_f32
        hi_ = A * math.log(2.0) * lg
        return sq, hi_ + CC + s * (2 * U * np.abs(hi_) + U * CC + U * np.abs(hi_ + CC))          # product, rounded a ln 2; rounded cc; the sum
    twelfth = 1.0 / 12.0
    sq_lo, lg_lo = pieces(lo, -1)
    sq_hi, lg_hi = pieces(hi, +1)
    below, above = hi < twelfth * (1 - U), lo > twelfth * (1 + U)          # the kernel compares with the rounded 1/12
    l = np.where(below, sq_lo, np.where(above, lg_lo, np.minimum(sq_lo, lg_lo)))
    h = np.where(below, sq_hi, np.where(above, lg_hi, np.maximum(sq_hi, lg_hi)))
    return l, h


def envelope(x, y):
    """The upper concave envelope of the points (x, y), x increasing, evaluated at x: the upper convex hull, interpolated."""
    hull = []
    for px, py in zip(x, y):
        while len(hull) >= 2 and (hull[-1][0] - hull[-2][0]) * (py - hull[-2][1]) >= (hull[-1][1] - hull[-2][1]) * (px - hull[-2][0]):
            hull.pop()
        hull.append((px, py))
    hx, hy = np.array(hull).T
    return np.interp(x, hx, hy)


def codes():
    """The grid of coded values: dense in [0, 1], denser towards black, the pieces' joins and their neighbours."""
    return np.unique(np.concatenate([np.linspace(0.0, 1.0, 65537), np.geomspace(1e-8, 1.0, 40001), 0.5 + np.linspace(-1e-6, 1e-6, 201)]))


def derive(name):
    """(max psi, the error in light of one decoded value; dc, the error of the coded mean of at most 8 samples)."""
    c = codes()
    lum = V.hdr_decode_host(c, name)
    d_lo, d_hi = decode_interval(name, c)
    psi = np.maximum(d_hi - lum, lum - d_lo)
    assert np.all(psi >= 0) and psi[0] < 1e-14, "a code within 2u of 0 decodes to next to no light (exact black: to exactly 0 on both sides)"
    order = np.argsort(lum, kind="stable")
    r, hat = lum[order], envelope(lum[order], np.maximum.accumulate(psi[order]))
    dr = hat + 8 * U * r
    e_lo, e_hi = encode_interval(name, r - dr, r + dr)
    back = V.hdr_encode_host(r, name)
    return float(psi.max()), float(np.maximum(e_hi - back, back - e_lo).max())


@pytest.fixture(scope="module")
def derived():
    return {name: derive(name) for name in NAMES}


def light_bound(psi):
    return 8 * psi + 35 * U + 8 * U


def bound_from(dc, mean, std):
    return max((dc + U) / s + 2 * U * max(m, 1.0 - m) / s for m, s in zip(mean, std))


@pytest.fixture(scope="module")
def bounds(derived):
    """{name: (B_LIGHT, bound(mean, std) -> float)}: what tests/test_hip_video_hdr.py asserts."""
    return {name: (light_bound(psi), lambda mean, std, dc=dc: bound_from(dc, mean, std)) for name, (psi, dc) in derived.items()}


# the derivation's values for the config's mean and std, rounded up (test_the_bounds_are_the_derivations holds them to it)
B = {"pq": 2.2e-4, "hlg": 3.4e-6}
B_LIGHT = {"pq": 1.1e-3, "hlg": 1.6e-5}


def test_the_bounds_are_the_derivations(derived):
    step10, step8 = (1 / 1023) / max(STD) / 4, (1 / 255) / max(STD) / 4          # a quarter of a code step in normalised units, smallest plane
    for name, (psi, dc) in derived.items():
        b, bl = bound_from(dc, MEAN, STD), light_bound(psi)
        print("%s: psi <= %.1f u, dc <= %.1f u = %.3g; B_LIGHT %.4g, B %.4g: a quarter of a 10-bit step is %.1f x B, of an 8-bit step %.1f x B"
              % (name, psi / U, dc / U, dc, bl, b, step10 / B[name], step8 / B[name]))
        assert b <= B[name] < 1.1 * b and bl <= B_LIGHT[name] < 1.1 * bl
    assert B["hlg"] < step10 / 100 and B["pq"] < step8 / 15, "far inside a quarter of a code step"
    assert B["pq"] < step10 / 4, "what the derivation reaches for PQ at 10 bits (the docstring says why no more)"


# ---- constants -------------------------------------------------------------------------------------------------------------------------
def test_rows_are_float64_constants_rounded_once():
    assert V.HDR_LIGHTS == ("pq", "hlg") and V.HDR_ROW == 8
    assert V.LIGHT_ROW == 9 and set(V.LIGHT_CURVES) == {"bt709", "srgb", "bt1886"} and V.SHUTTER_LIGHTS == ("coded",) + tuple(V.LIGHT_CURVES)
    m1, m2 = 2610 / 16384, 2523 / 4096 * 128
    c1, c2, c3 = 3424 / 4096, 2413 / 4096 * 32, 2392 / 4096 * 32
    a = 0.17883277
    b, cc = 1 - 4 * a, 0.5 - a * math.log(4 * a)
    want = {"pq": (0, [1 / m2, c1, c2, c3, 1 / m1, m1, m2, 0.0]),
            "hlg": (1, [1 / 3, math.log2(math.e) / a, cc, b, 1 / 12, a * math.log(2), 0.0, 0.0])}
    for name, (kind, vals) in want.items():
        k, row = V.hdr_light(name)
        assert k == kind and row.dtype == np.float32 and row.shape == (8,)
        assert [x.tobytes() for x in row] == [np.float32(x).tobytes() for x in vals], name
    assert all(float(np.float32(x)) == x for x in (m1, m2, c1, c2, c3)), "the PQ constants are exact in fp32"
    assert abs(c1 - (c3 - c2 + 1)) < 1e-15, "BT.2100: c1 = c3 - c2 + 1"
    for bad in ("srgb", "coded", "linear"):
        with pytest.raises(ValueError, match="'%s'" % bad):
            V.hdr_light(bad)
    with pytest.raises(ValueError, match="'pq'"):
        V.light_curve("pq")


def test_hlg_pieces_meet_in_value_and_slope():
    lo, hi = 0.5 ** 2 / 3, (math.exp((0.5 - CC) / A) + HB) / 12
    assert abs(lo - 1 / 12) < 1e-16 and abs(hi - 1 / 12) < 1e-15
    assert abs(2 * 0.5 / 3 - math.exp((0.5 - CC) / A) / (12 * A)) < 1e-14, "slopes dE/dc at c = 1/2"
    assert abs(math.sqrt(3 / 12) - 0.5) < 1e-16 and abs(A * math.log(12 / 12 - HB) + CC - 0.5) < 1e-15
    one = float(V.hdr_decode_host(1.0, "hlg"))
    print("hlg decode(1) = %.12g" % one)
    assert abs(one - 1.0) < 1e-7, "to the digits of a"
    assert float(V.hdr_decode_host(0.0, "hlg")) == 0.0 and float(V.hdr_encode_host(0.0, "hlg")) == 0.0
    # fp32: the row's pieces at the join, what the bound's union of the pieces covers
    d = V.hdr_decode_host(np.array([0.5, np.nextafter(np.float32(0.5), np.float32(1))], np.float32), "hlg", np.float32)
    assert abs(float(d[1]) - float(d[0])) < 1e-7


def test_pq_known_points():
    dec = lambda c: 10000.0 * float(V.hdr_decode_host(c, "pq"))
    enc = lambda nits: float(V.hdr_encode_host(nits / 10000.0, "pq"))
    assert dec(0.0) == 0.0 and dec(1.0) == 1.0 * 10000.0 and enc(0.0) == 0.0 and abs(enc(10000.0) - 1.0) < 1e-15
    print("pq: code 0.5 = %.4f cd/m2; 100 cd/m2 = code %.6f; 1000 cd/m2 = code %.6f; the formula at L = 0: %.4g"
          % (dec(0.5), enc(100.0), enc(1000.0), C1 ** M2))
    assert round(dec(0.5), 1) == 92.2 and round(enc(100.0), 3) == 0.508 and round(enc(1000.0), 3) == 0.752
    assert round(enc(100.0) * 1023) == 520 and round(enc(1000.0) * 1023) == 769, "full-range 10-bit codes of BT.2100's tables"
    assert 7.2e-7 < C1 ** M2 < 7.4e-7 and dec(C1 ** M2 * 0.999) == 0.0 and dec(1e-6) > 0.0


def test_the_issue_figures():
    """A PQ highlight at code 0.75 over black: the coded mean, a 2.4 gamma and the mean of light."""
    nits = lambda c: 10000.0 * float(V.hdr_decode_host(c, "pq"))
    light = (nits(0.75) + nits(0.0)) / 2
    code = float(V.hdr_encode_host(light / 10000.0, "pq"))
    g24 = 0.5 ** (1 / 2.4) * 0.75
    print("pq 0.75 = %.0f cd/m2; coded mean 0.375 = %.1f cd/m2; gamma-2.4 mean %.3f = %.1f cd/m2; mean of light %.0f cd/m2 = code %.3f"
          % (nits(0.75), nits(0.375), g24, nits(g24), light, code))
    assert 950 < nits(0.75) < 1000 and 15 < nits(0.375) < 25 and light / nits(0.375) > 20 and 0.66 < code < 0.70
    assert light / nits(g24) > 2, "a power law is no stand-in for PQ either"


@pytest.mark.parametrize("name", NAMES)
def test_decode_and_encode_are_inverse_and_monotone(name):
    c = np.linspace(0.0, 1.0, 4097)
    lum = V.hdr_decode_host(c, name)
    assert lum[0] == 0.0 and abs(lum[-1] - 1.0) < 1e-7 and np.all(np.diff(lum) > 0)
    back = V.hdr_encode_host(lum, name)
    # float64 rounding, carried by the steepest step: PQ's c = x ^ m2 turns 2^-53 of x into m2 = 79 times as much, and p - c1 near black
    # loses up to c1 / (p - c1) = 13 at c = 1 / 4096; HLG has nothing steeper than 12 / (12 E - b)
    tol = {"pq": 79 * 13 * 4 * 2.0 ** -53, "hlg": 64 * 2.0 ** -53}[name]
    print("%s: |encode(decode(c)) - c| <= %.3g (tolerance %.3g)" % (name, np.abs(back - c).max(), tol))
    assert np.abs(back - c).max() < tol


# ---- the yardstick -----------------------------------------------------------------------------------------------------------------------
def normalised(c, mean=MEAN, std=STD):
    m, s = (np.asarray(x, np.float32).reshape(1, 3, 1, 1) for x in (mean, std))
    return ((np.asarray(c, np.float32) - m) / s).astype(np.float32)


def run(frames, name, calls, scale, dtype=np.float64, encode=True):
    acc = np.full((1,) + frames.shape[1:], np.nan, dtype)
    cuts = np.linspace(0, frames.shape[0], calls + 1).astype(int)
    for i in range(calls):
        last = i == calls - 1
        assert V.accumulate_hdr_host(frames[cuts[i]:cuts[i + 1]], acc, i == 0, scale if last else 1.0, MEAN, STD, name, last and encode, dtype) is acc
    return acc


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("S,calls", [(1, 1), (3, 1), (8, 3)])
def test_copies_of_one_frame_give_it_back(name, S, calls):
    c = np.random.default_rng(S).uniform(0.001, 0.999, (1, 3, 9, 11))
    x = normalised(c)
    got = run(np.repeat(x, S, axis=0), name, calls, 1.0 / S)
    assert got.dtype == np.float64 and np.abs(got[0] - x[0].astype(np.float64)).max() < 1e-11


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_black_stays_exactly_black(name, dtype):
    m, s = np.float32(MEAN), np.float32(STD)
    black = ((np.float32(0.0) / np.float32(255.0) - m) / s).astype(np.float32)
    x = np.broadcast_to(black.reshape(1, 3, 1, 1), (5, 3, 4, 6)).copy()
    x[:, :, 2:, :] = normalised(np.random.default_rng(3).uniform(0, 1, (5, 3, 2, 6)))
    x[2, :, 0, 0] = -7.5
    got = run(x, name, 2, np.float32(0.2), dtype)
    want = ((dtype(0.0) - m.astype(dtype)) / s.astype(dtype)).reshape(3, 1, 1)
    assert np.array_equal(got[0, :, :2, :], np.broadcast_to(want, (3, 2, 6)))
    assert np.array_equal(got[0, :, :2, :].astype(np.float32), np.broadcast_to(black.reshape(3, 1, 1), (3, 2, 6)))
    assert np.all(run(x, name, 2, 1.0, dtype, encode=False)[0, :, :2, :] == 0.0)


@pytest.mark.parametrize("name", NAMES)
def test_values_outside_count_as_0_and_1_and_several_calls_equal_one(name):
    c = np.random.default_rng(2).uniform(-0.5, 1.5, (7, 3, 5, 7))
    c[0, :, 0, 0], c[1, :, 0, 0] = -3.0, 7.0
    x = normalised(c)
    one = run(x, name, 1, np.float32(1 / 7))
    assert np.abs(one - run(normalised(np.clip(c, 0.0, 1.0)), name, 1, np.float32(1 / 7))).max() < 1e-5
    for calls in (2, 7):
        assert np.array_equal(run(x, name, calls, np.float32(1 / 7)), one), "the same additions in the same order"


def test_float32_yardstick_lies_within_the_bounds():
    x = normalised(np.random.default_rng(5).uniform(0.0, 1.0, (8, 3, 16, 16)))
    x[:, :, 0:1, :4] = normalised(np.broadcast_to(np.float32([0.0, 1.0, 0.5, 1 / 1023]), (8, 3, 1, 4)))
    for name in NAMES:
        d = np.abs(run(x, name, 2, np.float32(0.125), np.float32).astype(np.float64) - run(x, name, 2, np.float32(0.125)))
        dl = np.abs(run(x, name, 2, 1.0, np.float32, encode=False).astype(np.float64) - run(x, name, 2, 1.0, encode=False))
        print("%s: float32 yardstick - float64 yardstick: %.3g at most (B = %.3g); in light %.3g (B_LIGHT = %.3g)"
              % (name, d.max(), B[name], dl.max(), B_LIGHT[name]))
        assert d.max() < B[name] and dl.max() < B_LIGHT[name]


# ---- BT.2020 -----------------------------------------------------------------------------------------------------------------------------
KR, KB = 0.2627, 0.0593
KG = 1.0 - KR - KB
BITS = (8, 10, 12, 16)


def test_tables():
    assert V.BT2020 not in (V.BT601, V.BT709) and V.MATRICES == {"bt601": V.BT601, "bt709": V.BT709, "bt2020": V.BT2020}
    assert [V.table_index(m) for m in (V.BT601, V.BT709, V.BT2020)] == [0, 1, 0] and V.default_matrix(2160) == V.BT709
    with pytest.raises(ValueError, match="unknown matrix 3"):
        V.table_index(3)
    for bits in (8, 9, 10, 12, 14, 16):
        t, own = V.yuv_table(bits), V.yuv_table(bits, V.BT2020)
        assert t.shape == (2, 2, V.YUV_ROW) and own.shape == (1, 2, V.YUV_ROW) and own.dtype == np.float32
        for m in (V.BT601, V.BT709):
            assert np.array_equal(V.yuv_table(bits, m).view(np.uint32), t.view(np.uint32))
        assert [x.tobytes() for x in own[0, 0, :9]] == [np.float32(x).tobytes() for x in (
            KR, KG, KB, 2 * (1 - KR), 2 * (1 - KB) * KB / KG, 2 * (1 - KR) * KR / KG, 2 * (1 - KB), 1 / (2 * (1 - KB)), 1 / (2 * (1 - KR)))]
        assert np.array_equal(own[0, :, 9:].view(np.uint32), t[0, :, 9:].view(np.uint32)), "ranges and depths do not depend on the matrix"
        assert V._table_ptr(bits, V.BT2020) is V._table_ptr(bits, V.BT2020) is not V._table_ptr(bits)
        assert V._table_ptr(bits, V.BT709) is V._table_ptr(bits)
    # the rows of BT.601 and BT.709 as they were before BT.2020: the 8-bit limited-range rows' bits, and the checksum of every depth
    t = V.yuv_table()
    assert t[V.BT601, V.LIMITED, :3].tobytes() == np.float32([0.299, 0.587, 0.114]).tobytes()
    assert t[V.BT709, V.LIMITED, :3].tobytes() == np.float32([0.2126, 0.7152, 0.0722]).tobytes()


def _planes(rgb8, bits, crange):
    """4:4:4 payload of R'G'B' in [0, 1] (shape [n, 3]) coded by the defining formulas in float64, unrounded: (Y, Cb, Cr) codes."""
    s, peak = float(1 << (bits - 8)), float((1 << bits) - 1)
    r, g, b = rgb8.T
    y = KR * r + KG * g + KB * b
    cb, cr = (b - y) / (2 * (1 - KB)), (r - y) / (2 * (1 - KR))
    if crange == V.LIMITED:
        return 219 * s * y + 16 * s, 224 * s * cb + 128 * s, 224 * s * cr + 128 * s
    return peak * y, peak * cb + 128 * s, peak * cr + 128 * s


def _canvas(rgb, mean=MEAN, std=STD):
    """[n, 3] R'G'B' in [0, 1] -> one normalised fp32 canvas [1,3,32,32] with the n pixels in the first row of a 1 x n crop... as 4:4:4 h = 1."""
    n = rgb.shape[0]
    x = np.zeros((1, 3, 32, 32 * ((n + 31) // 32)), np.float32)
    top, left = (32 - 1) // 2, (x.shape[3] - n) // 2
    for p in range(3):
        x[0, p, top, left:left + n] = (np.float32(rgb[:, p]) - np.float32(mean[p])) / np.float32(std[p])
    return x


@pytest.mark.parametrize("crange", [V.LIMITED, V.FULL])
@pytest.mark.parametrize("bits", BITS)
def test_primaries_greys_and_colours_through_444(bits, crange):
    s, peak = float(1 << (bits - 8)), float((1 << bits) - 1)
    # primaries land where Kr, Kg, Kb say
    prim = np.eye(3)
    got = V.frames_to_yuv_host(_canvas(prim), 1, 3, V.C444, V.BT2020, crange, bits=bits)
    y = V.split_planes(got if bits > 8 else got, 1, 3, V.C444, bits)[0].reshape(-1).astype(np.float64)
    want = np.array([KR, KG, KB]) * (219 * s if crange == V.LIMITED else peak) + (16 * s if crange == V.LIMITED else 0)
    assert np.abs(y - want).max() <= 0.5 + 1e-3 * s, (y, want)
    # legal greys: Y codes over the legal range with neutral chroma come back exactly; so do in-gamut colours made from R'G'B' codes
    ylo, yhi = (16 * s, 235 * s) if crange == V.LIMITED else (0.0, peak)
    ys = np.unique(np.round(np.linspace(ylo, yhi, 257)))
    rng = np.random.default_rng(bits + crange)
    rgb = rng.uniform(0.02, 0.98, (256, 3))
    yc, cbc, crc = (np.round(p) for p in _planes(rgb, bits, crange))
    yq = np.concatenate([ys, yc])
    uq = np.concatenate([np.full(ys.size, 128 * s), cbc])
    vq = np.concatenate([np.full(ys.size, 128 * s), crc])
    n = yq.size
    words = np.concatenate([yq, uq, vq]).astype(np.uint8 if bits == 8 else "<u2")
    payload = words.view(np.uint8).reshape(1, -1)
    assert payload.shape[1] == V.frame_bytes(1, n, V.C444, bits)
    x = V.yuv_to_frames_host(payload, 1, n, V.C444, V.BT2020, crange, bits=bits)
    back = V.frames_to_yuv_host(x, 1, n, V.C444, V.BT2020, crange, bits=bits)
    assert np.array_equal(back, payload), "4:4:4 codes of greys and in-gamut colours are fixed points of decode and encode"
    # the fp32 ingest against a float64 evaluation of the defining formulas: the bounds tests/test_video_cpu.py uses for the other matrices
    k = (255.0 / (219 * s), 255.0 / (224 * s), 16 * s) if crange == V.LIMITED else (255.0 / peak, 255.0 / peak, 0.0)
    yl, cb, cr = (yq - k[2]) * k[0], (uq - 128 * s) * k[1], (vq - 128 * s) * k[1]
    ref = np.stack([yl + 2 * (1 - KR) * cr, yl - 2 * (1 - KB) * KB / KG * cb - 2 * (1 - KR) * KR / KG * cr, yl + 2 * (1 - KB) * cb])
    top, left = (x.shape[2] - 1) // 2, (x.shape[3] - n) // 2
    for p in range(3):
        want = (np.clip(ref[p], 0, 255) / 255.0 - np.float64(np.float32(MEAN[p]))) / np.float64(np.float32(STD[p]))
        assert np.abs(x[0, p, top, left:left + n] - want).max() < 2e-5


# ---- options -------------------------------------------------------------------------------------------------------------------------------
class _Cfg:
    def getint(self, section, key):
        return 2


def test_constructor():
    for name in NAMES:
        assert V.parse_shutter_light(name) == name
        vi = V.VideoInterpolator(None, _Cfg(), target_rate=(24, 1), shutter="1/2", shutter_light=name, matrix=V.BT2020)
        assert vi.shutter_light == name and vi.matrix == V.BT2020
        with pytest.raises(ValueError, match="shutter_light='%s'.*give a shutter" % name):
            V.VideoInterpolator(None, _Cfg(), target_rate=(24, 1), shutter_light=name)
    with pytest.raises(ValueError, match="'linear'"):
        V.VideoInterpolator(None, _Cfg(), target_rate=(24, 1), shutter="1/2", shutter_light="linear")
    with pytest.raises(ValueError, match="unknown matrix 7"):
        V.VideoInterpolator(None, _Cfg(), matrix=7)
    assert V.VideoInterpolator(None, _Cfg()).matrix is None


BASE = ["-c", "x.ini", "--expt", "e", "--log", "l", "--input", "-", "--output", "-"]


def test_cli(capsys):
    import evaluate_video
    import interpolate_video as cli
    for name in NAMES:
        a = cli.getargs(BASE + ["--fps", "24", "--shutter", "180", "--shutter_light", name, "--matrix", "bt2020"])
        assert a.shutter_light == name and V.MATRICES[a.matrix] == V.BT2020
        with pytest.raises(SystemExit) as e:
            cli.getargs(BASE + ["--fps", "24", "--shutter_light", name])
        assert e.value.code == 2 and "--shutter_light %s is the light in which --shutter averages" % name in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.getargs(BASE + ["--fps", "24", "--shutter", "180", "--shutter_light", "linear"])
    assert "'linear'" in capsys.readouterr().err
    assert cli.getargs(BASE).matrix is None
    argv = [x for x in BASE if x not in ("--output", "-")][:6] + ["--input", "-", "--hold", "2", "--matrix", "bt2020"]
    assert evaluate_video.getargs(argv).matrix == "bt2020"
