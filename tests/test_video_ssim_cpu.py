"""SSIM and the frame-mix baseline of the hold-out score without a GPU (ssm_amd/video_score.py): the numpy yardsticks of ssm_plane_ssim_fwd
and ssm_payload_mix_fwd against exact second evaluations in Python integers and fractions, the kernel's division by multiply-shift over
every numerator the scorer can reach, and the report with the options off against today's text."""
import math
from fractions import Fraction

import numpy as np
import pytest

CENTRED, COSITED, C444, C422 = 0, 1, 2, 3
LAYOUTS = (CENTRED, COSITED, C444, C422)
ONE = 1 << 32


def S():
    from ssm_amd import video_score
    return video_score


def V():
    from ssm_amd import video
    return video


def payloads(h, w, layout, bits, n=2, seed=0, smooth=False):
    """n payloads of random samples of `bits` significant bits; smooth: a ramp plus a little noise, so that windows correlate."""
    v = V()
    rng = np.random.RandomState(100 * h + w + 7 * layout + bits + 1000 * seed)
    count = v.frame_bytes(h, w, layout, bits) // v.sample_bytes(bits)
    peak = (1 << bits) - 1
    if smooth:
        x = (np.arange(count) * 37 % (peak + 1))[None] + rng.randint(0, max(2, peak // 16), size=(n, count))
        x = np.minimum(x, peak)
    else:
        x = rng.randint(0, peak + 1, size=(n, count))
    return np.ascontiguousarray(x.astype(np.uint8 if bits == 8 else "<u2")).view(np.uint8).reshape(n, -1)


def round_half_even(fr):
    """The nearest integer of a Fraction, ties to even; and whether it was a tie."""
    fl = math.floor(fr)
    rest = fr - fl
    if rest == Fraction(1, 2):
        return (fl if fl % 2 == 0 else fl + 1), True
    return (fl if rest < Fraction(1, 2) else fl + 1), False


def exact_plane(a, b, bits):
    """The second evaluation: a loop over the windows of one plane (lists of rows of Python ints): (sum of fx*, count, the least distance
    of q 2^32 from a tie, the largest factor)."""
    c1, c2 = S().ssim_constants(bits)
    rows, cols = len(a), len(a[0])
    nby, nbx = rows >> 2, cols >> 2
    total, count, clear, biggest = 0, 0, Fraction(1), 0
    for wy in range(nby - 1):
        for wx in range(nbx - 1):
            s1 = s2 = ss = s12 = 0
            for y in range(4 * wy, 4 * wy + 8):
                for x in range(4 * wx, 4 * wx + 8):
                    u, v = a[y][x], b[y][x]
                    s1, s2, ss, s12 = s1 + u, s2 + v, ss + u * u + v * v, s12 + u * v
            var, covar = 64 * ss - s1 * s1 - s2 * s2, 64 * s12 - s1 * s2
            f0, f1, f2, f3 = 2 * s1 * s2 + c1, 2 * covar + c2, s1 * s1 + s2 * s2 + c1, var + c2
            assert f2 > 0 and f3 > 0
            biggest = max(biggest, abs(f0), abs(f1), f2, f3)
            scaled = Fraction(f0 * f1, f2 * f3) * ONE
            fx, tie = round_half_even(scaled)
            assert not tie
            clear = min(clear, abs(scaled - math.floor(scaled) - Fraction(1, 2)))
            total += fx
            count += 1
    return total, count, clear, biggest


# The float64 evaluation against the exact one.  With u = 2^-53: fl(f0 f1) = f0 f1 (1 + d1), fl(f2 f3) = f2 f3 (1 + d2), the quotient adds
# (1 + d3), all |d| <= u (the factors themselves are exact doubles, below 2^53): q = q* (1 + d1)(1 + d3) / (1 + d2), |q / q* - 1| <= 3 u +
# O(u^2) < 3 * 2^-53 * (1 + 2^-50).  |q*| <= 1 + 2^-8 (Cauchy-Schwarz gives |f0 f1| <= f2 f3 up to the constants' share), so |q 2^32 - q* 2^32|
# < 3 * 2^-53 * 2^32 * 1.01 < 2^-19; the scaling by 2^32 is exact.  Hence fx and fx* differ by at most 1, and only where q* 2^32 lies within
# 2^-19 of a tie; per plane |sum fx - sum fx*| <= count.  On the inputs below every window stays further than 2^-19 from a tie (asserted),
# so the sums are EQUAL.
TIE_MARGIN = Fraction(1, 1 << 19)


@pytest.mark.parametrize("bits", [8, 10, 16])
@pytest.mark.parametrize("smooth", [False, True])
@pytest.mark.parametrize("h,w", [(8, 8), (9, 13), (45, 71)])
def test_yardstick_against_the_exact_second_evaluation(h, w, bits, smooth):
    s, v = S(), V()
    layout = C444 if (h, w) != (45, 71) else CENTRED          # 45 x 71 in 4:2:0: chroma 23 x 36, unaligned, trailing rows and columns
    pl = payloads(h, w, layout, bits, n=2, smooth=smooth)
    a, b = pl[0:1], pl[1:2]
    got = s.plane_ssim_host(a, b, h, w, layout, bits)
    assert got.dtype == np.int64 and got.shape == (1, 3)
    counts = s.plane_windows(h, w, layout)
    near_ties = []
    for p, (pa, pb) in enumerate(zip(v.split_planes(a, h, w, layout, bits), v.split_planes(b, h, w, layout, bits))):
        total, count, clear, biggest = exact_plane(pa[0].tolist(), pb[0].tolist(), bits)
        assert count == counts[p] and biggest < 1 << (29 if bits == 8 else 45)
        assert abs(int(got[0, p]) - total) <= count
        if clear <= TIE_MARGIN:
            near_ties.append((p, clear))
        else:
            assert int(got[0, p]) == total, (p, int(got[0, p]), total)
    assert not near_ties, "inputs of this test that come within 2^-19 of a tie: %r" % (near_ties,)
    assert s.plane_ssim_host(b, a, h, w, layout, bits).tolist() == got.tolist(), "symmetric"


def test_one_payload_broadcasts_against_many():
    s = S()
    h, w = 9, 13
    pl = payloads(h, w, C444, 8, n=4)
    rows = [s.plane_ssim_host(pl[i:i + 1], pl[3:4], h, w, C444, 8)[0].tolist() for i in range(3)]
    assert s.plane_ssim_host(pl[:3], pl[3:4], h, w, C444, 8).tolist() == rows == s.plane_ssim_host(pl[3:4], pl[:3], h, w, C444, 8).tolist()


def test_constants_and_factors_at_the_16_bit_extremes():
    s = S()
    assert s.ssim_constants(8) == (416, 235963), "x264's ssim_c1 and ssim_c2"
    for bits in (8, 10, 12, 16):
        peak = (1 << bits) - 1
        c1, c2 = s.ssim_constants(bits)
        assert c1 == math.floor(Fraction(peak * peak * 64, 10000) + Fraction(1, 2)) and c1 == int(.01 * .01 * peak * peak * 64 + .5)
        assert c2 == math.floor(Fraction(9 * peak * peak * 64 * 63, 10000) + Fraction(1, 2))
    # the largest factors of a window of words: every sample 65535 on both sides, and 0 against 65535
    c1, c2 = s.ssim_constants(16)
    m = 65535
    for u, v in ((m, m), (0, m), (m, 0)):
        s1, s2, ss, s12 = 64 * u, 64 * v, 64 * (u * u + v * v), 64 * u * v
        fs = (2 * s1 * s2 + c1, 2 * (64 * s12 - s1 * s2) + c2, s1 * s1 + s2 * s2 + c1, 64 * ss - s1 * s1 - s2 * s2 + c2)
        assert all(abs(f) < 1 << 45 for f in fs) and (1 << 45) < (1 << 53)
    # a checkerboard of 0 and 65535 against its inverse: the largest variance and the most negative covariance
    ss, s12, s1 = 64 * m * m, 0, 32 * m
    assert 64 * ss - 2 * s1 * s1 + c2 < 1 << 45 and abs(2 * (64 * s12 - s1 * s1) + c2) < 1 << 45


@pytest.mark.parametrize("bits", [8, 16])
def test_identical_planes_score_exactly_one_and_a_checkerboard_against_its_inverse_is_negative(bits):
    s, v = S(), V()
    h, w = 20, 28
    for layout in LAYOUTS:
        a = payloads(h, w, layout, bits, n=2)
        counts = s.plane_windows(h, w, layout)
        assert s.plane_ssim_host(a, a, h, w, layout, bits).tolist() == [[c * ONE for c in counts]] * 2
    peak = (1 << bits) - 1
    yy, xx = np.mgrid[0:h, 0:w]
    board = ((yy + xx) & 1) * peak
    dt = np.uint8 if bits == 8 else "<u2"
    a = np.concatenate([board.ravel()] * 3).astype(dt).view(np.uint8)[None]
    b = np.concatenate([(peak - board).ravel()] * 3).astype(dt).view(np.uint8)[None]
    got = s.plane_ssim_host(a, b, h, w, C444, bits)[0]
    assert all(int(x) < 0 for x in got), got
    assert s.ssim_value(int(got[0]), s.plane_windows(h, w, C444)[0]) < -0.99


def test_trailing_columns_and_rows_belong_to_no_block():
    s = S()
    h, w = 10, 15          # 2 x 3 blocks, 1 x 2 windows; columns 12..14 and rows 8..9 are trailing
    a, b = payloads(h, w, C444, 8, n=1), payloads(h, w, C444, 8, n=1, seed=1)
    ref = s.plane_ssim_host(a, b, h, w, C444, 8).tolist()
    for y, x in ((0, 12), (3, 14), (8, 0), (9, 14)):
        c = b.copy()
        c[0, y * w + x] ^= 0xff
        assert s.plane_ssim_host(a, c, h, w, C444, 8).tolist() == ref, (y, x)
    c = b.copy()
    c[0, 7 * w + 11] ^= 0xff          # the last covered sample
    assert s.plane_ssim_host(a, c, h, w, C444, 8)[0, 0] != ref[0][0]


def test_plane_windows():
    s = S()
    want = {(2, 2): {CENTRED: (0, 0, 0), COSITED: (0, 0, 0), C444: (0, 0, 0), C422: (0, 0, 0)},
            (4, 6): {CENTRED: (0, 0, 0), COSITED: (0, 0, 0), C444: (0, 0, 0), C422: (0, 0, 0)},
            (7, 100): {CENTRED: (0, 0, 0), COSITED: (0, 0, 0), C444: (0, 0, 0), C422: (0, 0, 0)},
            (8, 8): {CENTRED: (1, 0, 0), COSITED: (1, 0, 0), C444: (1, 1, 1), C422: (1, 0, 0)},
            (45, 71): {CENTRED: (10 * 16, 4 * 8, 4 * 8), COSITED: (160, 32, 32), C444: (160, 160, 160), C422: (160, 10 * 8, 10 * 8)}}
    for (h, w), by_layout in want.items():
        for layout, counts in by_layout.items():
            assert s.plane_windows(h, w, layout) == counts, (h, w, layout)
            for bits in (8, 16):
                z = np.zeros((1, V().frame_bytes(h, w, layout, bits)), np.uint8)
                assert s.plane_ssim_host(z, z, h, w, layout, bits).tolist() == [[c * ONE for c in counts]]


def test_ssim_value_and_db():
    s = S()
    assert s.ssim_value(5 * ONE, 5) == 1.0 and s.ssim_db(1.0) == math.inf
    assert s.ssim_value(-ONE, 2) == -0.5 and math.isnan(s.ssim_value(0, 0))
    assert abs(s.ssim_db(0.9) - 10.0) < 1e-12 and abs(s.ssim_db(0.99) - 20.0) < 1e-9


# ---- the cross-fade -------------------------------------------------------------------------------------------------------------------
def half_up(a, b, k, den):
    """Round-half-up of the exact rational (a (den - k) + b k) / den, in Python integers."""
    n = a * (den - k) + b * k
    return (2 * n + den) // (2 * den)          # floor(n / den + 1/2) = floor((2 n + den) / (2 den)), integers throughout


@pytest.mark.parametrize("den", [2, 3, 7, 8, 255])
def test_mix_yardstick_on_the_whole_byte_grid(den):
    s = S()
    a = np.repeat(np.arange(256, dtype=np.uint8), 256)[None]
    b = np.tile(np.arange(256, dtype=np.uint8), 256)[None]
    ks = sorted(set([0, 1, den // 2, den - 1, den]))
    for k in ks:
        got = s.payload_mix_host(a, b, 1, k, 0, den, 8)
        assert got.dtype == np.uint8 and got.shape == a.shape
        x, y = a[0].astype(object), b[0].astype(object)
        want = [(2 * (int(u) * (den - k) + int(v) * k) + den) // (2 * den) for u, v in zip(x, y)]          # floor(r + 1/2), exact
        assert got[0].tolist() == want, (den, k)
    assert half_up(3, 4, 1, 2) == 4 and half_up(255, 0, 1, 3) == 170 and s.payload_mix_host(a, b, 1, 0, 0, den, 8).tolist() == a.tolist()
    assert s.payload_mix_host(a, b, 1, den, 0, den, 8).tolist() == b.tolist(), "k = den gives b"
    rows = s.payload_mix_host(a, b, den + 1, 0, 1, den, 8)          # rows k = 0 .. den of one call, both operands broadcast
    assert rows.shape == (den + 1, 65536) and rows[0].tolist() == a[0].tolist() and rows[den].tolist() == b[0].tolist()


def test_mix_yardstick_on_random_words_at_the_largest_den():
    s = S()
    den = 65535
    rng = np.random.RandomState(3)
    a, b = (rng.randint(0, 65536, size=100000).astype("<u2") for _ in range(2))
    a[:4], b[:4] = (0, 65535, 65535, 0), (65535, 0, 65535, 0)
    a8, b8 = a.view(np.uint8)[None], b.view(np.uint8)[None]
    for k in (0, 1, 32767, 32768, 65534, 65535):
        got = s.payload_mix_host(a8, b8, 1, k, 0, den, 16).view("<u2")[0].tolist()
        assert got == [half_up(int(u), int(v), k, den) for u, v in zip(a.tolist(), b.tolist())], k
    assert s.payload_mix_host(a8, b8, 1, 0, 0, den, 16).tolist() == a8.tolist() and s.payload_mix_host(a8, b8, 1, den, 0, den, 16).tolist() == b8.tolist()


def test_the_kernels_multiply_shift_division_is_exact_on_every_reachable_numerator():
    """ssm_payload_mix_fwd divides by mix_divisor(den)'s pair.  8 bits: the scorer passes den = hold in 2..256 and the numerator a (den - k) +
    b k + den // 2 is at most 255 den + den // 2: every numerator from 0 to there, for every den.  16 bits: the ends of the range, the
    neighbourhood of every multiple of den that 2^32 allows to sample, and random numerators, for small, odd, power-of-two and large dens."""
    s = S()
    for den in range(2, 257):
        x = np.arange(255 * den + den // 2 + 1, dtype=np.uint64)
        assert np.array_equal(s.mix_divide(x, den), x // np.uint64(den)), den
    rng = np.random.RandomState(9)
    for den in (2, 3, 5, 7, 8, 255, 256, 257, 1023, 4095, 32767, 32768, 32769, 65521, 65534, 65535):
        top = 65535 * den + den // 2
        assert top < 1 << 32
        m, shift = s.mix_divisor(den)
        assert 0 < m < 1 << 32 and 0 <= shift < 16
        mult = rng.randint(0, 65536, size=20000).astype(np.uint64) * np.uint64(den)
        x = np.concatenate([np.arange(0, min(top, 200000) + 1, dtype=np.uint64), np.arange(max(0, top - 200000), top + 1, dtype=np.uint64),
                            mult, mult + np.uint64(den - 1), mult[mult > 0] - np.uint64(1),
                            rng.randint(0, top + 1, size=200000).astype(np.uint64)])
        x = x[x <= top]
        assert np.array_equal(s.mix_divide(x, den), x // np.uint64(den)), den
    x = np.array([0, 1, (1 << 32) - 1, (1 << 32) - 2, 1 << 31], dtype=np.uint64)          # the theorem covers all 32 bits
    for den in (2, 3, 641, 65535):
        assert np.array_equal(s.mix_divide(x, den), x // np.uint64(den))


# ---- the report with the options off -------------------------------------------------------------------------------------------------
def rows_of_the_existing_test():
    s = S()
    res = s.HoldOutResult(4, 8, (100, 25, 25))
    res.frames_read, res.kept, res.trailing = 11, 3, 2
    res.frames = [(1, 1, (100, 25, 0), (400, 25, 25)), (2, 2, (200, 50, 25), (900, 25, 25)), (3, 3, (0, 0, 0), (100, 0, 25))]
    return res


TODAY_STATS = ['n:1 k:1 mse_y 1.000000 psnr_y 48.1308 psnr_u 48.1308 psnr_v inf psnr_avg 48.9226 nearest_psnr_y 42.1102',
               'n:2 k:2 mse_y 2.000000 psnr_y 45.1205 psnr_u 45.1205 psnr_v 48.1308 psnr_avg 45.4984 nearest_psnr_y 38.5884',
               'n:3 k:3 mse_y 0.000000 psnr_y inf psnr_u inf psnr_v inf psnr_avg inf nearest_psnr_y 48.1308']
TODAY_TABLE = "\n".join(['hold-out score, hold = 4: 11 frames read, 3 kept, 3 scored, 2 trailing and not scored (PSNR in dB of the pooled MSE, peak 255)',
                         'k      frames |  model_y  model_u  model_v model_avg |   near_y   near_u   near_v near_avg',
                         '1/4         1 |   48.131   48.131      inf   48.923 |   42.110   48.131   48.131   43.360',
                         '2/4         1 |   45.121   45.121   48.131   45.498 |   38.588   48.131   48.131   40.114',
                         '3/4         1 |      inf      inf      inf      inf |   48.131      inf   48.131   48.923',
                         'all         3 |   48.131   48.131   52.902   48.642 |   41.441   49.892   48.131   42.830',
                         'worst frame: PSNR-Y 45.121 dB at input frame 2'])


def test_report_with_the_options_off_is_todays_text():
    res = rows_of_the_existing_test()
    assert res.stats_lines() == TODAY_STATS
    assert res.table() == TODAY_TABLE
    assert sorted(res.pooled()) == ["frames", "model", "nearest"] and res.more == [] and res.columns == ("model", "nearest")


def test_report_with_the_options_on_appends():
    s = S()
    res = rows_of_the_existing_test()
    on = s.HoldOutResult(4, 8, (100, 25, 25), windows=(6, 1, 1), ssim=True, mix=True)
    on.frames_read, on.kept, on.trailing, on.frames = res.frames_read, res.kept, res.trailing, list(res.frames)
    one = {"model": (6 * ONE, ONE, ONE), "nearest": (3 * ONE, 0, -ONE), "mix": (3 * ONE, ONE, ONE)}
    on.more = [{"sse": {"mix": (100, 25, 0)}, "ssim": one} for _ in on.frames]
    table = on.table().split("\n")
    assert table[:len(TODAY_TABLE.split("\n"))] == TODAY_TABLE.split("\n"), "the first lines are the default table's"
    assert any("mix_y" in ln and "mix_avg" in ln for ln in table) and any("model_y" in ln and "near_avg" in ln and "mix_avg" in ln for ln in table[8:])
    lines = on.stats_lines()
    assert [ln[:len(t)] for ln, t in zip(lines, TODAY_STATS)] == TODAY_STATS
    assert lines[0].endswith(" mix_psnr_y 48.1308 mix_psnr_avg %.4f ssim_y 1.000000 ssim_u 1.000000 ssim_v 1.000000 ssim_avg 1.000000"
                             " nearest_ssim_y 0.500000 mix_ssim_y 0.500000" % s.psnr(125, 150, 8))
    p = on.pooled()
    assert sorted(p) == ["frames", "mix", "model", "nearest", "ssim"] and p["mix"]["y"] == s.psnr(300, 300, 8)
    assert p["ssim"]["model"] == {"y": 1.0, "u": 1.0, "v": 1.0, "avg": 1.0}
    assert p["ssim"]["nearest"] == {"y": 0.5, "u": 0.0, "v": -1.0, "avg": 0.25}, "avg pools by windows: (3 + 0 - 1) / 8"
    only = s.HoldOutResult(4, 8, (100, 25, 25), windows=(6, 1, 1), ssim=True)
    only.frames, only.more = list(res.frames), [{"ssim": {"model": one["model"], "nearest": one["nearest"]}} for _ in res.frames]
    assert sorted(only.pooled(2)) == ["frames", "model", "nearest", "ssim"] and sorted(only.pooled(2)["ssim"]) == ["model", "nearest"]


def test_cli_parsing_of_the_new_options():
    import evaluate_video as E
    base = ["-c", "cfg.ini", "--expt", "e", "--log", "run.log", "--input", "in.y4m", "--hold", "8"]
    a = E.getargs(base)
    assert (a.ssim, a.mix) == (False, False)
    a = E.getargs(base + ["--ssim", "--mix"])
    assert (a.ssim, a.mix) == (True, True)
