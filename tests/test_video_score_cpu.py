"""Hold-out scoring without a GPU (ssm_amd/video_score.py): the numpy yardstick of ssm_plane_sse_fwd on planes worked out by hand, PSNR
and its pooling, which frames are kept, held out and left over, the command line and the stats line."""
import math

import numpy as np
import pytest

CENTRED, COSITED, C444, C422 = 0, 1, 2, 3


def S():
    from ssm_amd import video_score
    return video_score


def V():
    from ssm_amd import video
    return video


def dims(h, w, layout):
    return (h, w) if layout == C444 else ((h, (w + 1) // 2) if layout == C422 else ((h + 1) // 2, (w + 1) // 2))


@pytest.mark.parametrize("bits", [8, 10, 16])
@pytest.mark.parametrize("layout", [CENTRED, COSITED, C444, C422])
@pytest.mark.parametrize("h,w", [(2, 2), (3, 5), (45, 71), (4, 6)])
def test_yardstick_on_hand_computed_planes(h, w, layout, bits):
    """a = 0 everywhere; b's plane p is the constant p + 1 except its first sample (+ 2) and its last (+ 3): the sums follow from the
    plane's size alone, and a plane boundary put one sample off would move them."""
    s, v = S(), V()
    ch, cw = dims(h, w, layout)
    sizes = (h * w, ch * cw, ch * cw)
    assert s.plane_samples(h, w, layout) == sizes
    dt = np.uint8 if bits == 8 else "<u2"
    scale = 1 if bits == 8 else 200          # words: values past one byte
    planes, want = [], []
    for p, n in enumerate(sizes):
        x = np.full(n, (p + 1) * scale, dtype=np.int64)
        x[0] += 2
        x[-1] += 3
        planes.append(x)
        want.append(int((x * x).sum()))
    b = np.concatenate(planes).astype(dt).view(np.uint8)[None]
    a = np.zeros_like(b)
    assert b.shape[1] == v.frame_bytes(h, w, layout, bits)
    got = s.plane_sse_host(a, b, h, w, layout, bits)
    assert got.dtype == np.uint64 and got.shape == (1, 3) and got.tolist() == [want]
    assert s.plane_sse_host(b, a, h, w, layout, bits).tolist() == [want]
    assert s.plane_sse_host(b, b, h, w, layout, bits).tolist() == [[0, 0, 0]]
    three = np.concatenate([a, b, a])
    assert s.plane_sse_host(three, b, h, w, layout, bits).tolist() == [want, [0, 0, 0], want], "one payload against three"


def test_yardstick_counts_all_16_bits_and_does_not_overflow():
    s = S()
    h, w = 3, 5
    fb = V().frame_bytes(h, w, C444, 16)
    a, b = np.zeros((2, fb), np.uint8), np.full((2, fb), 255, np.uint8)
    assert s.plane_sse_host(a, b, h, w, C444, 10).tolist() == [[15 * 65535 ** 2] * 3] * 2, "the depth does not mask the words"
    assert 15 * 65535 ** 2 > 1 << 35


def test_psnr_and_pooling():
    s = S()
    assert s.psnr(0, 100, 8) == math.inf and s.psnr_avg((0, 0, 0), (4, 1, 1), 8) == math.inf
    assert s.psnr(65025 * 7, 7, 8) == 0.0, "every sample off by the peak: 0 dB"
    assert s.psnr(100, 100, 8) == 10.0 * math.log10(255.0 ** 2)
    assert abs(s.psnr(1023 ** 2 * 6, 6, 10)) < 1e-12 and s.psnr(6, 6, 10) == 10.0 * math.log10(1023 ** 2), "peak of 10 bits is 1023"
    assert abs(s.psnr(6, 6, 10) - 60.1975) < 1e-3
    # two frames of 100 samples, MSE 1 and 100: the pooled PSNR is that of MSE 50.5, not the mean of 48.13 and 28.13 dB
    one, two = s.psnr(100, 100, 8), s.psnr(10000, 100, 8)
    pooled = s.psnr(100 + 10000, 200, 8)
    assert abs(pooled - 10.0 * math.log10(65025 / 50.5)) < 1e-12 and abs(pooled - (one + two) / 2) > 6.9
    # planes pooled by sums as well: a perfect chroma does not make the average infinite
    assert s.psnr_avg((400, 0, 0), (400, 100, 100), 8) == s.psnr(400, 600, 8)
    res = s.HoldOutResult(2, 8, (100, 25, 25))
    res.frames = [(1, 1, (100, 0, 50), (400, 25, 25)), (3, 1, (10000, 25, 0), (100, 0, 0))]
    p = res.pooled()
    assert p["frames"] == 2 and p["model"]["y"] == pooled and p["model"]["u"] == s.psnr(25, 50, 8)
    assert p["model"]["avg"] == s.psnr(10175, 300, 8) and p["nearest"]["y"] == s.psnr(500, 200, 8)
    assert res.pooled(1) == p and res.worst() == (two, 3)


def brute(n, hold):
    kept = [i for i in range(n) if i % hold == 0]
    held = [(i, i % hold) for i in range(n) if i % hold and i < kept[-1]]
    return kept, held, [i for i in range(n) if i > kept[-1]]


@pytest.mark.parametrize("hold", [2, 3, 4, 5])
def test_kept_held_and_trailing_frames(hold):
    s = S()
    for n in range(1, 21):
        kept, held, trailing = s.hold_out_plan(n, hold)
        assert (kept, held, trailing) == brute(n, hold), n
        assert len(trailing) == (n - 1) % hold and len(kept) + len(held) + len(trailing) == n
        for i, k in held:          # the nearer kept frame: the left one below the middle, the right one from the middle on
            left = sum(1 for kk in range(1, hold) if 2 * kk < hold)
            assert s.nearest_split(hold) == left
    assert s.hold_out_plan(0, hold) == ([], [], [])
    for bad in (1, 0, -2, 2.5, True):
        with pytest.raises(ValueError, match="hold must be a whole number, at least 2"):
            s.hold_out_plan(5, bad)


def test_stats_lines_and_table():
    s = S()
    res = s.HoldOutResult(4, 8, (100, 25, 25))
    res.frames_read, res.kept, res.trailing = 11, 3, 2
    res.frames = [(1, 1, (100, 25, 0), (400, 25, 25)), (2, 2, (200, 50, 25), (900, 25, 25)), (3, 3, (0, 0, 0), (100, 0, 25))]
    lines = res.stats_lines()
    assert lines[0] == "n:1 k:1 mse_y 1.000000 psnr_y 48.1308 psnr_u 48.1308 psnr_v inf psnr_avg %.4f nearest_psnr_y 42.1102" % s.psnr(125, 150, 8)
    assert lines[2] == "n:3 k:3 mse_y 0.000000 psnr_y inf psnr_u inf psnr_v inf psnr_avg inf nearest_psnr_y 48.1308"
    import re
    pat = re.compile(r"n:\d+ k:\d+ mse_y \S+ psnr_y \S+ psnr_u \S+ psnr_v \S+ psnr_avg \S+ nearest_psnr_y \S+")
    assert all(pat.fullmatch(ln) for ln in lines)
    table = res.table().split("\n")
    assert "11 frames read, 3 kept, 3 scored, 2 trailing and not scored" in table[0] and "peak 255" in table[0]
    assert table[1].split()[:2] == ["k", "frames"] and "model_y" in table[1] and "near_avg" in table[1]
    assert [ln.split()[0] for ln in table[2:6]] == ["1/4", "2/4", "3/4", "all"]
    assert table[6] == "worst frame: PSNR-Y %.3f dB at input frame 2" % s.psnr(200, 100, 8)
    empty = s.HoldOutResult(4, 8, (100, 25, 25))
    assert "nothing scored" in empty.table() and empty.pooled() is None and empty.worst() is None


def test_cli_parsing():
    import evaluate_video as E
    base = ["-c", "cfg.ini", "--expt", "e", "--log", "run.log", "--input", "in.y4m"]
    a = E.getargs(base + ["--hold", "8"])
    assert (a.hold, a.stats, a.output, a.matrix, a.color_range, a.flow_scale, a.tile) == (8, None, None, None, None, 1, None)
    a = E.getargs(base + ["--hold", "4", "--stats", "f.log", "--output", "o.y4m", "--matrix", "bt601", "--range", "full", "--tile", "64x96",
                          "--halo", "32", "--blend", "8"])
    assert (a.hold, a.stats, a.output, a.matrix, a.color_range, a.tile, a.halo, a.blend) == (4, "f.log", "o.y4m", "bt601", "full", (64, 96), 32, 8)
    assert E.getargs(base + ["--hold", "2", "--flow_scale", "2"]).flow_scale == 2
    for bad in (base, base + ["--hold", "1"], base + ["--hold", "x"], base + ["--hold", "2", "--fps", "60"], base + ["--hold", "2", "--speed", "1/2"],
                base + ["--hold", "2", "--shutter", "180"], base + ["--hold", "2", "--scene_cut", "0.1"], base + ["--hold", "2", "--upsample_rate", "4"],
                base + ["--hold", "2", "--output", "-", "--stats", "-"]):
        with pytest.raises(SystemExit):
            E.getargs(bad)


def test_a_ring_without_a_writer_takes_the_rows_and_drops_them():
    v = V()
    taken = []

    def rows():
        taken.append("pass")
        yield b"x"

    with v.PassRing(2, None) as ring:
        r = ring.take()
        ring.hand(r, None, rows)
        ring.hand(None, None, [b"y"])
    assert taken == ["pass"] and not ring.failure
