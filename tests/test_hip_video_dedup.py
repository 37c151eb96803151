"""Repeated frames on the GPU: ssm_block_sad_fwd against block_sad_host word for word, and VideoInterpolator(dedup=),
scripts/interpolate_video.py --dedup, against the fixed grid on the clip without its repeats and against the reference call of
tests/test_hip_video_timeline.py (ingest -> FullModel.interpolate at the pair's times, padded to `slots` -> egress).

The moving clip of tests/video_clips.py holds no repeat under the default thresholds at this size (tests/test_video_dedup_cpu.py asserts
it), so dedup=True is used wherever the defaults are meant; the clips' repeats are exact copies unless a test says otherwise."""
import io
import os
import sys
from fractions import Fraction as Fr

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from video_clips import (LAYOUTS, V, bits_of, clip_file, clip_payloads, deep_payloads, fbytes, frames_of, random_payloads, read_clip,  # noqa: E402
                         synthetic_model, y4m)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
H, W = 64, 96          # the frame of tests/test_hip_video_timeline.py
SIZES = ((8, 8), (16, 24), (17, 23), (40, 72), (144, 528))          # the last: 3 x 3 tiles of Y and, in 4:2:0, 2 x 2 of U and V


# ---- the kernel ----------------------------------------------------------------------------------------------------------------------------
def words(a, b, h, w, layout, sb, lo=None, out=None):
    """block_sad of device tensors -> the words as numpy uint64 [N, 3, 2]."""
    got = V().block_sad(a, b, h, w, layout, bits_of(sb), lo, out=out)
    torch.cuda.synchronize()
    return got.cpu().numpy().view(np.uint64)


def check(a, b, h, w, layout, sb, lo=None):
    """Kernel == yardstick on numpy payloads a, b; returns the words."""
    want = V().block_sad_host(a, b, h, w, layout, bits_of(sb), lo)
    got = words(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), h, w, layout, sb, lo)
    assert got.shape == want.shape and np.array_equal(got, want), (h, w, layout, sb, lo, got.tolist(), want.tolist())
    return got


@pytest.mark.parametrize("sb", [1, 2])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_kernel_equals_the_yardstick(layout, sb):
    for h, w in SIZES:
        a, b = random_payloads(h, w, layout, sb, 3, seed=1), random_payloads(h, w, layout, sb, 3, seed=2)
        got = check(a, b, h, w, layout, sb)
        assert got[:, 0, 0].min() > 0
        lo = int(got[1, 0, 0])          # a block's own d: that block is not over, every larger one is
        for x in (0, lo, lo - 1):
            check(a, b, h, w, layout, sb, x)
        # all-0 against all-255 / all-65535: d at its maximum, every block over any lo below it
        zero, full = np.zeros_like(a[:1]), np.full_like(a[:1], 255)
        top = 64 * (255 if sb == 1 else 65535)
        got = check(zero, full, h, w, layout, sb, top - 1)
        counts = V().block_counts(h, w, layout)
        assert got[0].tolist() == [[top if c else 0, c] for c in counts]
        assert check(zero, full, h, w, layout, sb, top)[0, :, 1].tolist() == [0, 0, 0]
        # a difference in the last block of the last plane only (and, where V has no block, in none)
        c = a.copy()
        v = V().split_planes(c, h, w, layout, bits_of(sb))[2]
        v[:, 8 * (v.shape[1] >> 3) - 1, 8 * (v.shape[2] >> 3) - 1] ^= 1
        got = check(a, c, h, w, layout, sb, 0)
        assert got[0].tolist() == [[0, 0], [0, 0], [1, 1] if counts[2] else [0, 0]]


@pytest.mark.parametrize("sb", [1, 2])
def test_operand_forms_and_the_cleared_result(sb):
    """Rows n + 1 and n of one buffer, stride 0, a negative stride, payloads inside wider rows; `out` prefilled; two runs."""
    v = V()
    for (h, w), layout in (((17, 23), v.CENTRED), ((40, 72), v.C422), ((144, 528), v.CENTRED)):
        fb = fbytes(h, w, layout, sb)
        clip = random_payloads(h, w, layout, sb, 5, seed=3)
        clip[2] = clip[1]
        dev = torch.from_numpy(clip).to(DEV)
        args = (h, w, layout, bits_of(sb))
        out = torch.ones(4, 3, 2, dtype=torch.int64, device=DEV)
        got = words(dev[1:], dev[:-1], h, w, layout, sb, 0, out=out)
        assert np.array_equal(got, v.block_sad_host(clip[1:], clip[:-1], *args, 0)), "rows n + 1 and n; the entry clears `out`"
        assert got[1].tolist() == [[0, 0]] * 3
        assert np.array_equal(words(dev[1:], dev[:-1], h, w, layout, sb, 0, out=out), got), "two runs give equal words"
        assert np.array_equal(words(dev[:1].expand(5, -1), dev, h, w, layout, sb), v.block_sad_host(clip[:1], clip, *args)), "stride 0"
        from ssm_amd import hipbind as hb
        o = torch.empty(5, 3, 2, dtype=torch.int64, device=DEV)          # a_n = frame 4 - n: the last row and a negative stride
        hb.check(hb.load().ssm_block_sad_fwd(dev[4].data_ptr(), dev.data_ptr(), -dev.stride(0), dev.stride(0), 5, h, w, layout, sb,
                                             v.DEDUP_LO << (8 * (sb - 1)), o.data_ptr(), hb.stream_ptr()))
        torch.cuda.synchronize()
        assert np.array_equal(o.cpu().numpy().view(np.uint64), v.block_sad_host(clip[::-1], clip, *args)), "a negative stride"
        wide = torch.zeros(5, fb + 6, dtype=torch.uint8, device=DEV)          # rows of another pitch, starting 2 bytes in
        wide[:, 2:2 + fb] = dev
        assert np.array_equal(words(wide[1:, 2:], wide[:-1, 2:], h, w, layout, sb), v.block_sad_host(clip[1:], clip[:-1], *args))


# ---- the stream ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    return synthetic_model(DEV)


def run(m, cfg, payloads, h=H, w=W, chroma="420jpeg", reader=None, **kw):
    """The clip through VideoInterpolator(**kw): (the frames written, vi.repeats)."""
    v = V()
    r = reader if reader is not None else v.Y4MReader(clip_file(payloads, h, w, chroma))
    sink = io.BytesIO()
    wr = v.Y4MWriter.like(sink, r)
    vi = v.VideoInterpolator(m, cfg, **kw)
    count = vi.run(r, wr)
    assert count == wr.frames_written
    return frames_of(sink.getvalue()), list(vi.repeats)


def expected(m, cfg, base, gaps, rate, slots, h=H, w=W, siting=0):
    """The reference call of tests/test_hip_video_timeline.py for the pairs (i, i + 1) of `base` with gap gaps[i] at upsample_rate `rate`:
    the originals as their own bytes, between them the frames at t = j / (g rate) from one call of `slots` times per pair."""
    v = V()
    dev = torch.from_numpy(base).to(DEV)
    matrix, crange = v.default_matrix(h), v.LIMITED
    out = [base[0]]
    for i, g in enumerate(gaps):
        ts = [float(v.Timeline.t32(Fr(j, g * rate))) for j in range(1, g * rate)]
        if ts:
            x = v.frames_from_yuv(dev[i:i + 2], h, w, siting, matrix, crange, cfg, True)
            frames = m.interpolate(x[None], ts + [ts[-1]] * (slots - len(ts)))
            out += list(v.frames_to_yuv(frames[:len(ts)], h, w, siting, matrix, crange, cfg).cpu().numpy())
        out.append(base[i + 1])
    return np.stack(out)


@pytest.fixture(scope="module")
def base():
    return clip_payloads(5, H, W, 0)


@pytest.mark.parametrize("g", [2, 3])
def test_every_frame_repeated_g_times_is_the_base_clip_at_rate_g(model, base, g):
    cfg, m = model
    clip = np.repeat(base, g, axis=0)
    got, repeats = run(m, cfg, clip, upsample_rate=1, dedup=True, dedup_max=g - 1)
    want, none = run(m, cfg, base, upsample_rate=g)
    assert none == [] and want.shape[0] == 4 * g + 1 and got.shape[0] == 5 * g
    assert repeats == [(1 + g * i, g - 1, True, 0, 0) for i in range(4)] + [(4 * g + 1, g - 1, False, 0, 0)]
    assert np.array_equal(got[:4 * g + 1], want), int((got[:4 * g + 1] != want).sum())
    assert all(np.array_equal(x, base[4]) for x in got[4 * g + 1:]), "the run at the clip's end stays: copies of the last frame"
    assert not np.array_equal(got[1], base[0]) and not np.array_equal(got[1], base[1]), "a repeat's place holds a synthesised frame"


GAPS = (2, 3, 1, 2)


@pytest.fixture(scope="module")
def gapped(model, base):
    """The clip with gaps 2, 3, 1, 2 and its output at N = 2, one pair per pass: computed once, read by two tests."""
    cfg, m = model
    clip = np.concatenate([np.repeat(base[i:i + 1], g, axis=0) for i, g in enumerate(GAPS)] + [base[4:]])
    return clip, run(m, cfg, clip, upsample_rate=2, dedup=True)


def test_mixed_gaps_at_rate_2_equal_the_reference_call(model, base, gapped):
    cfg, m = model
    clip, (got, repeats) = gapped
    assert clip.shape[0] == 9 and got.shape[0] == 17
    assert repeats == [(1, 1, True, 0, 0), (3, 2, True, 0, 0), (7, 1, True, 0, 0)]
    want = expected(m, cfg, base, GAPS, 2, 5)
    assert np.array_equal(got[[0, 4, 10, 12, 16]], base), "frames that stay are their own bytes, on the input's grid"
    assert np.array_equal(got, want), int((got != want).sum())
    assert len({x.tobytes() for x in got}) == 17, "no output is a copy of another"


def test_two_pairs_per_pass(model, gapped):
    cfg, m = model
    clip, (ref, repeats) = gapped
    got, again = run(m, cfg, clip, upsample_rate=2, dedup=True, pairs_per_batch=2)
    assert again == repeats and got.shape == ref.shape
    diff = np.abs(got.astype(int) - ref.astype(int))          # the bound of tests/test_hip_video_timeline.py test_two_pairs_per_pass, for its reason
    print("two pairs per pass: %d codes differ, by %d at most" % (int((diff != 0).sum()), int(diff.max())))
    assert diff.max() <= 1


def test_a_clip_without_repeats_is_the_run_without_the_option(model):
    cfg, m = model
    clip = clip_payloads(6, H, W, 0)
    got, repeats = run(m, cfg, clip, upsample_rate=2, dedup=True)
    want, _ = run(m, cfg, clip, upsample_rate=2)
    diff = got.astype(int) - want.astype(int)
    print("no repeats: %d codes differ, by %d at most" % (int((diff != 0).sum()), int(np.abs(diff).max())))
    assert repeats == [] and np.array_equal(got, want)


def test_a_still_and_a_run_at_the_end_stay_as_they_are(model, base):
    cfg, m = model
    clip = np.stack([base[0], base[1], base[1], base[1], base[1], base[2], base[3], base[3]])          # a run of D + 1 = 3; a run at the end
    got, repeats = run(m, cfg, clip, upsample_rate=2, dedup=True)
    want, _ = run(m, cfg, clip, upsample_rate=2)
    diff = got.astype(int) - want.astype(int)
    print("stills: %d codes differ, by %d at most" % (int((diff != 0).sum()), int(np.abs(diff).max())))
    assert repeats == [(2, 3, False, 0, 0), (7, 1, False, 0, 0)]
    assert np.array_equal(got, want)


def test_near_repeats(model, base):
    cfg, m = model
    v = V()
    rng = np.random.RandomState(11)

    def near(x):          # +-1 on a third of the samples: block sums of at most 64, far under lo = 320
        d = rng.randint(-1, 2, size=x.shape) * (rng.randint(0, 3, size=x.shape) == 0)
        return np.clip(x.astype(int) + d, 16, 235).astype(np.uint8)

    clip = np.stack([base[0], near(base[0]), base[1], base[2], near(base[2]), near(base[2]), base[3]])
    other = clip.copy()
    other[1], other[4], other[5] = near(base[0]), near(base[2]), near(base[2])
    assert not np.array_equal(clip, other)
    got, repeats = run(m, cfg, clip, upsample_rate=1, dedup=True)
    assert [r[:3] for r in repeats] == [(1, 1, True), (4, 2, True)] and 0 < repeats[1][3] <= 64 and repeats[1][4] == 0
    assert np.array_equal(got[[0, 2, 3, 6]], base[:4]) and not any(np.array_equal(got[k], clip[k]) for k in (1, 4, 5))
    again, _ = run(m, cfg, other, upsample_rate=1, dedup=True)
    assert np.array_equal(again, got), "the repeats' own bytes reach nothing"
    exact, repeats = run(m, cfg, clip, upsample_rate=1, dedup=(0, 0, 0))
    assert repeats == [] and np.array_equal(exact, clip), "under (0, 0, 0) a near copy is a frame of its own"


def test_422p10_clip(model):
    cfg, m = model
    v = V()
    h, w, tag = 40, 56, "422p10"
    b = deep_payloads(3, h, w, tag)
    clip = np.stack([b[0], b[0], b[1], b[2]])
    got, repeats = run(m, cfg, None, reader=v.Y4MReader(y4m(clip, h, w, tag), extended=True), upsample_rate=1, dedup=True, dedup_max=1)
    want, _ = run(m, cfg, None, reader=v.Y4MReader(y4m(b, h, w, tag), extended=True), upsample_rate=2)
    assert repeats == [(1, 1, True, 0, 0)] and got.shape[0] == 4
    assert np.array_equal(got[:3], want[:3]) and np.array_equal(got[3], b[2])
    assert not np.array_equal(got[1], b[0])


def test_detelecine_then_dedup(model):
    """A telecined clip whose film repeats one frame: pulldown removal upstream hands on the film, the repeat is repaired in it."""
    cfg, m = model
    v = V()
    h, w = 40, 56
    f = clip_payloads(11, h, w, 0)
    film = np.stack([f[0], f[1], f[2], f[3], f[4], f[5], f[5], f[6], f[7], f[8], f[9], f[10]])
    video = v.telecine_host(film, h, w)
    back, _ = v.detelecine_host(video, h, w)
    assert np.array_equal(back, film[:len(back)]) and len(back) >= 8, "the cadence survives the repeat (host definition)"
    src = v.TelecineSource(v.Y4MReader(clip_file(video, h, w), interlaced=True), DEV)
    got, repeats = run(m, cfg, None, reader=src, upsample_rate=1, dedup=True)
    want, same = run(m, cfg, back, h, w, upsample_rate=1, dedup=True)
    assert repeats == same == [(6, 1, True, 0, 0)]
    assert np.array_equal(got, want) and np.array_equal(got[:6], film[:6]) and not np.array_equal(got[6], film[6])


def test_bytes_do_not_depend_on_the_chunk(model, gapped):
    """RepeatSource alone, chunks of 1, 2 and 5 frames: the frames handed on, their gaps and the log are those of dedup_host."""
    v = V()
    clip, _ = gapped
    acts, rep = v.dedup_host(clip, H, W)
    kept = [n for n, a in acts if a is None]
    for chunk in (1, 2, 5):
        src = v.RepeatSource(v.Y4MReader(clip_file(clip, H, W)), DEV, True, 2, frames_per_chunk=chunk)
        buf, frames, gaps = np.empty(src.frame_bytes, np.uint8), [], []
        while src.read_frame_into(buf):
            frames.append(buf.copy())
            gaps.append((src.gap, src.next_gap))
        assert np.array_equal(np.stack(frames), clip[kept]) and src.repeats == rep.log
        assert gaps == [(0, 2), (2, 3), (3, 1), (1, 2), (2, 0)]


def test_cli_end_to_end(model, tmp_path, caplog):
    import logging

    import interpolate_video
    cfg, m = model
    h, w = 40, 56
    b = clip_payloads(3, h, w, 0)
    clip = np.stack([b[0], b[0], b[1], b[1], b[1], b[2]])
    src, dst, ini, logf = (str(tmp_path / x) for x in ("in.y4m", "out.y4m", "cfg.ini", "log.txt"))
    with open(src, "wb") as f:
        f.write(clip_file(clip, h, w).getvalue())
    with open(ini, "w") as f:
        cfg.write(f)
    argv = ["-c", ini, "--expt", "t", "--log", logf, "--input", src, "--output", dst, "--upsample_rate", "2", "--dedup", "--dedup_max", "1"]
    with caplog.at_level(logging.INFO):
        assert interpolate_video.main(argv, model=m) == 11
    hdr, got = read_clip(dst)
    assert got.shape[0] == 11 and hdr.rate == (60, 1)
    assert np.array_equal(got[[0, 4, 6, 8, 10]], clip[[0, 2, 3, 4, 5]]), "frames that stay, the still's among them, are their own bytes"
    assert not any(np.array_equal(got[2], p) for p in clip), "the repeat's place holds a synthesised frame"
    text = "\n".join(r.getMessage() for r in caplog.records if "dedup" in r.getMessage())
    assert "dedup: 1 repeat from input frame 1: repaired; worst block sum 0" in text
    assert "dedup: 2 repeats from input frame 3: left as they are (a still)" in text and "dedup: 2 runs, 1 repaired" in text


def test_device_memory_is_flat_in_clip_length(model, base):
    cfg, m = model
    v = V()
    vi = v.VideoInterpolator(m, cfg, upsample_rate=1, dedup=True, dedup_max=1)
    peaks = []
    for n in (4, 4, 12):          # the first run also builds the plans
        clip = np.repeat(clip_payloads(n, H, W, 0), 2, axis=0)
        r = v.Y4MReader(clip_file(clip, H, W))
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(DEV)
        sink = open(os.devnull, "wb")
        assert vi.run(r, v.Y4MWriter.like(sink, r)) == 2 * n
        sink.close()
        assert len(vi.repeats) == n and sum(1 for x in vi.repeats if x[2]) == n - 1
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated(DEV))
    print("peak device memory: 8 frames %d B, 24 frames %d B" % (peaks[1], peaks[2]))
    assert peaks[2] <= peaks[1], peaks
