"""Scene cuts of the streamed video path on the GPU: ssm_luma_sad_fwd against its numpy yardstick (ssm_amd.video.
luma_sad_host) - every sum EQUAL, the kernel is integer arithmetic - and VideoInterpolator(scene_cut=) on the clip of
tests/video_cut_clips.py, whose one cut and its room on either side of the threshold tests/test_video_cuts_cpu.py holds through the yardstick:
the cut pair's output frames are input frames' own bytes, `cuts` carries the yardstick's score, every other frame is byte for byte the
frame of the run without the option, and without the option the loop is the composition it was."""
import io
import logging
import os
import sys
from fractions import Fraction as Fr

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import video_cut_clips as C  # noqa: E402
from video_clips import S, V, clip_file, random_payloads, read_clip, synthetic_model  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
# (h, w) with N = 3 planes each.  64 x 96: every plane on a 16-byte boundary, whole 16-byte pieces.  4 x 6: less than one piece.
# 130 x 1030: 133900 bytes = 8 spans of 16 KiB and a part, the last piece 12 bytes; frame 0 takes the unguarded whole-span loads, frames 1
# and 2 (200850 bytes apart) the byte loads.  45 x 71: frame_bytes = 4851 is odd, frame 1 starts at an odd address.  46 x 70: even, no
# multiple of 16.  Then the span cases of tests/test_hip_video_score.py, for the one-plane form of the kernel the two entry points share:
# 128 x 256 = two spans exactly, 99 x 331 = two spans and one byte, 129 x 127 = a span less one byte.
SPAN = 16384
assert 128 * 256 == 2 * SPAN and 99 * 331 == 2 * SPAN + 1 and 129 * 127 == SPAN - 1
KERNEL_SIZES = ((64, 96), (4, 6), (130, 1030), (45, 71), (46, 70), (128, 256), (99, 331), (129, 127))
ONES = (1 << 64) - 1


def payloads_ab(h, w, n=3, seed=0):
    """Two sets of n payloads in the 4:2:0 layout with random Y planes; the chroma bytes that follow each Y plane are 0 in a and 255 in b,
    so that any byte read past a plane changes a sum."""
    v = V()
    fb = v.frame_bytes(h, w, 0)
    rng = np.random.RandomState(100 * h + w + seed)
    a, b = rng.randint(0, 256, size=(n, fb)).astype(np.uint8), rng.randint(0, 256, size=(n, fb)).astype(np.uint8)
    a[:, h * w:], b[:, h * w:] = 0, 255
    return a, b


def sad(a, b, h, w):
    """The device op on numpy payloads, `sums` filled with ones before the call; the sums as Python integers."""
    v = V()
    out = torch.full((a.shape[0],), -1, dtype=torch.int64, device=DEV)
    got = v.luma_sad(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), h, w, out=out)
    assert got is out
    return out.cpu().numpy().view(np.uint64).tolist()


def want(a, b, h, w):
    return V().luma_sad_host(a[:, :h * w].reshape(-1, h, w), b[:, :h * w].reshape(-1, h, w)).tolist()


@pytest.mark.parametrize("h,w", KERNEL_SIZES)
def test_kernel_equals_its_yardstick(h, w):
    a, b = payloads_ab(h, w)
    assert len({bytes(p[:h * w]) for p in np.concatenate([a, b])}) == 6, "distinct planes per n"
    ref = want(a, b, h, w)
    assert len(set(ref)) == 3
    assert sad(a, b, h, w) == ref
    assert sad(b, a, h, w) == ref
    assert sad(a, a, h, w) == [0, 0, 0]
    assert sad(a[1:2], b[1:2], h, w) == ref[1:2], "N = 1, the plane at frame 1's address"


@pytest.mark.parametrize("h,w", [(64, 96), (45, 71)])
def test_full_range_and_nothing_read_past_a_plane(h, w):
    fb = V().frame_bytes(h, w, 0)
    a, b = np.zeros((3, fb), np.uint8), np.full((3, fb), 255, np.uint8)
    assert sad(a, b, h, w) == [255 * h * w] * 3 == sad(b, a, h, w)


@pytest.mark.parametrize("h,w", [(64, 96), (45, 71)])
def test_operands_may_be_views_of_one_buffer(h, w):
    v = V()
    a, _ = payloads_ab(h, w, n=4, seed=1)
    buf = torch.from_numpy(a).to(DEV)
    out = torch.full((3,), -1, dtype=torch.int64, device=DEV)
    v.luma_sad(buf[:-1], buf[1:], h, w, out=out)
    assert out.cpu().numpy().view(np.uint64).tolist() == want(a[:-1], a[1:], h, w)
    wide = buf[::2]          # frames 0 and 2: a row stride of two frames
    assert wide.stride(0) == 2 * a.shape[1]
    assert v.luma_sad(wide, buf[1::2], h, w).cpu().numpy().view(np.uint64).tolist() == want(a[::2], a[1::2], h, w)


@pytest.mark.parametrize("h,w", [(45, 71), (99, 331)])
def test_one_kernel_under_luma_sad_and_plane_sse(h, w):
    """ssm_luma_sad_fwd and ssm_plane_sse_fwd launch one span-sum kernel: with one plane per payload, sums[n], and with three, sums[3 n +
    p].  On the same 8-bit 4:2:0 operands - three payloads against three, against one row of b, and one row of a against three, which
    plane_sse takes as a 0-stride expand and luma_sad, which refuses stride 0, as three calls of N = 1 - each equals its own numpy
    yardstick.  The two meet through the yardsticks alone: over the Y plane sum |d| <= sum d^2 <= 255 sum |d|, of one parity."""
    v, s = V(), S()
    a, b = random_payloads(h, w, 0, 1), random_payloads(h, w, 0, 1, seed=1)
    fb = a.shape[1]
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    for xa, xb, ha, hb_ in ((ta, tb, a, b), (ta, tb[1:2].expand(3, fb), a, b[[1, 1, 1]]), (ta[2:3].expand(3, fb), tb, a[[2, 2, 2]], b)):
        want_sad, want_sse = want(ha, hb_, h, w), s.plane_sse_host(ha, hb_, h, w, 0, 8).tolist()
        assert len(set(want_sad)) == 3 and len({row[0] for row in want_sse}) == 3, "a pair booked under another n would show"
        sse = torch.full((3, 3), -1, dtype=torch.int64, device=DEV)
        s.plane_sse(xa, xb, h, w, 0, 8, out=sse)
        assert sse.cpu().numpy().view(np.uint64).tolist() == want_sse
        if xa.stride(0) and xb.stride(0):
            got = v.luma_sad(xa, xb, h, w, out=torch.full((3,), -1, dtype=torch.int64, device=DEV))
        else:
            got = torch.cat([v.luma_sad(xa[n:n + 1], xb[n:n + 1], h, w, out=torch.full((1,), -1, dtype=torch.int64, device=DEV)) for n in range(3)])
        assert got.cpu().numpy().view(np.uint64).tolist() == want_sad
        for sad_n, (sse_y, _, _) in zip(want_sad, want_sse):
            assert sad_n <= sse_y <= 255 * sad_n and (sse_y - sad_n) % 2 == 0


def test_refusals_by_name():
    from ssm_amd import hipbind as hb
    lib = hb.load()
    h, w, n = 8, 12, 2
    a = torch.zeros(n, 200, dtype=torch.uint8, device=DEV)
    b = torch.ones(n, 200, dtype=torch.uint8, device=DEV)
    sums = torch.full((4,), -1, dtype=torch.int64, device=DEV)

    def call(**kw):
        x = dict(a=a.data_ptr(), b=b.data_ptr(), sa=200, sb=200, n=n, h=h, w=w, sums=sums.data_ptr())
        x.update(kw)
        hb.check(lib.ssm_luma_sad_fwd(x["a"], x["b"], x["sa"], x["sb"], x["n"], x["h"], x["w"], x["sums"], hb.stream_ptr()))

    call()
    torch.cuda.synchronize()
    assert sums.cpu().numpy().view(np.uint64).tolist() == [h * w, h * w, ONES, ONES], "N words are written, no more"
    for bad, text in ((dict(a=None), "null pointer"), (dict(b=None), "null pointer"), (dict(sums=None), "null pointer"),
                      (dict(n=0), r"N=0 outside 1\.\.65535"), (dict(n=65536), r"N=65536 outside 1\.\.65535"),
                      (dict(h=0), "bad plane size 0x12"), (dict(w=-1), "bad plane size 8x-1"),
                      (dict(sa=95), r"strides 95 \(a\), 200 \(b\) shorter than the plane's 96 bytes"),
                      (dict(sb=-95), r"strides 200 \(a\), -95 \(b\) shorter than the plane's 96 bytes"),
                      (dict(sums=sums.data_ptr() + 4), "sums is not 8-byte aligned")):
        with pytest.raises(RuntimeError, match=text):
            call(**bad)
    sums.fill_(-1)
    call(sa=-200, a=a.data_ptr() + 200, n=2)          # a negative stride is an address like any other; with N = 1 no stride is looked at
    call(sa=0, sb=1, n=1, sums=sums.data_ptr() + 16)
    torch.cuda.synchronize()
    assert sums.cpu().numpy().view(np.uint64).tolist() == [h * w, h * w, h * w, ONES]


# ---- the streamed loop ------------------------------------------------------------------------------------------------------------------
RATE = 4


@pytest.fixture(scope="module")
def model():
    return synthetic_model(DEV)


def run(m, cfg, payloads, h, w, **kw):
    """The clip through VideoInterpolator(**kw): (its frames, its `cuts`)."""
    v = V()
    r = v.Y4MReader(clip_file(payloads, h, w))
    sink = io.BytesIO()
    wr = v.Y4MWriter.like(sink, r, rate=kw.get("target_rate") or r.rate)
    vi = v.VideoInterpolator(m, cfg, n_streams=2, **kw)
    count = vi.run(r, wr)
    _, got = read_clip(io.BytesIO(sink.getvalue()))
    assert got.shape[0] == count == wr.frames_written
    return got, vi.cuts


_plain = {}


def plain(model, h, w, pb, **mode):
    """The run without the option, once per (size, pairs_per_batch, mode)."""
    cfg, m = model
    key = (h, w, pb, tuple(sorted(mode.items())))
    if key not in _plain:
        got, cuts = run(m, cfg, C.cut_clip(h, w), h, w, pairs_per_batch=pb, **mode)
        assert cuts == []
        _plain[key] = got
    return _plain[key]


@pytest.mark.parametrize("pb", [1, 2])
@pytest.mark.parametrize("h,w", C.SIZES)
def test_fixed_grid(model, h, w, pb):
    """upsample_rate 4: output 4 i + s is step s of pair i.  Pair (4, 5) opens a pass at both pairs_per_batch (passes take frames 1-2, 3-4,
    5-6 at two pairs): its left frame was uploaded by the pass before."""
    cfg, m = model
    payloads = C.cut_clip(h, w)
    ref = plain(model, h, w, pb, upsample_rate=RATE)
    got, cuts = run(m, cfg, payloads, h, w, pairs_per_batch=pb, upsample_rate=RATE, scene_cut=C.THRESHOLD)
    assert got.shape == ref.shape and got.shape[0] == (C.N_FRAMES - 1) * RATE + 1
    assert cuts == [(C.CUT, C.pair_scores(payloads, h, w)[C.CUT][2])]
    o = RATE * C.CUT
    assert np.array_equal(got[o + 1], payloads[C.CUT]), "t = 1/4: the left frame's bytes"
    assert np.array_equal(got[o + 2], payloads[C.CUT + 1]) and np.array_equal(got[o + 3], payloads[C.CUT + 1]), "t = 1/2, 3/4: the right frame's"
    assert not any(np.array_equal(ref[o + s], p) for s in (1, 2, 3) for p in payloads), "without the option the pair's frames are synthesised"
    rest = [k for k in range(got.shape[0]) if k not in (o + 1, o + 2, o + 3)]
    assert np.array_equal(got[rest], ref[rest]), int((got[rest] != ref[rest]).sum())


@pytest.mark.parametrize("pb", [1, 2])
@pytest.mark.parametrize("h,w", C.SIZES)
def test_timeline(model, h, w, pb):
    """30 -> 75 frames/s: step 2/5, output k at tau = 2 k / 5.  Every pair runs; pair (4, 5) gets k = 11 (t = 2/5) and k = 12 (t = 4/5)."""
    cfg, m = model
    payloads = C.cut_clip(h, w)
    ref = plain(model, h, w, pb, target_rate=(75, 1))
    got, cuts = run(m, cfg, payloads, h, w, pairs_per_batch=pb, target_rate=(75, 1), scene_cut=C.THRESHOLD)
    assert got.shape == ref.shape and got.shape[0] == 23
    assert cuts == [(C.CUT, C.pair_scores(payloads, h, w)[C.CUT][2])]
    assert np.array_equal(got[11], payloads[C.CUT]) and np.array_equal(got[12], payloads[C.CUT + 1])
    assert not any(np.array_equal(ref[k], p) for k in (11, 12) for p in payloads)
    rest = [k for k in range(23) if k not in (11, 12)]
    assert np.array_equal(got[rest], ref[rest]), int((got[rest] != ref[rest]).sum())


def test_a_threshold_nothing_reaches_changes_nothing(model):
    """The sums are taken and the rows decided on the writer thread, and the stream is the one without the option."""
    cfg, m = model
    h, w = C.SIZES[1]
    got, cuts = run(m, cfg, C.cut_clip(h, w), h, w, pairs_per_batch=2, upsample_rate=RATE, scene_cut=1)
    assert cuts == [] and np.array_equal(got, plain(model, h, w, 2, upsample_rate=RATE))


def test_without_the_option_the_loop_is_the_composition_it_was(model):
    """scene_cut=None against ingest -> FullModel.interpolate -> egress pair by pair (fixed grid) and pair by pair at the timeline's times
    padded to `slots` (tests/test_hip_video.py, tests/test_hip_video_timeline.py hold the same composition on their clips)."""
    from ssm_amd.evaluation import t_values
    cfg, m = model
    v = V()
    h, w = C.SIZES[0]
    payloads = C.cut_clip(h, w)
    dev = torch.from_numpy(payloads).to(DEV)
    matrix, crange = v.default_matrix(h), v.LIMITED
    planes = v.frames_from_yuv(dev, h, w, 0, matrix, crange, cfg, True)
    fixed = [payloads[0]]
    for i in range(C.N_FRAMES - 1):
        frames = m.interpolate(planes[i:i + 2][None], t_values(RATE))
        fixed.extend(v.frames_to_yuv(frames, h, w, 0, matrix, crange, cfg).cpu().numpy())
        fixed.append(payloads[i + 1])
    got = plain(model, h, w, 1, upsample_rate=RATE)
    assert np.array_equal(got, np.stack(fixed)), int((got != np.stack(fixed)).sum())
    tl = v.Timeline(Fr(2, 5))
    timed = []
    for i in range(C.N_FRAMES - 1):
        ts = [float(v.Timeline.t32(t)) for t in tl.times(i)]
        frames = m.interpolate(planes[i:i + 2][None], ts + [ts[-1]] * (tl.slots - len(ts)))
        made = list(v.frames_to_yuv(frames[:len(ts)], h, w, 0, matrix, crange, cfg).cpu().numpy())
        timed.extend(([payloads[i]] if tl.on_frame(i) is not None else []) + made)
    assert tl.on_frame(C.N_FRAMES - 1) is None and len(timed) == 23
    got = plain(model, h, w, 1, target_rate=(75, 1))
    assert np.array_equal(got, np.stack(timed)), int((got != np.stack(timed)).sum())


def test_cli_logs_each_cut(model, tmp_path, caplog):
    import interpolate_video
    cfg, m = model
    h, w = C.SIZES[1]
    payloads = C.cut_clip(h, w)[2:8]          # 6 frames, the cut between frames 2 and 3
    src, dst, ini, logf = (str(tmp_path / x) for x in ("in.y4m", "out.y4m", "cfg.ini", "log.txt"))
    with open(src, "wb") as f:
        f.write(clip_file(payloads, h, w).getvalue())
    with open(ini, "w") as f:
        cfg.write(f)
    argv = ["-c", ini, "--expt", "t", "--log", logf, "--input", src, "--output", dst, "--upsample_rate", "2", "--scene_cut", "1/10"]
    with caplog.at_level(logging.INFO):
        assert interpolate_video.main(argv, model=m) == 11
    _, got = read_clip(dst)
    assert np.array_equal(got[5], payloads[3]), "t = 1/2 of the cut pair: the right frame"
    assert np.array_equal(got[::2], payloads)
    lines = [r.getMessage() for r in caplog.records if "scene cut" in r.getMessage()]
    assert len(lines) == 1 and "scene cut between input frames 2 and 3: score" in lines[0] and "(threshold 1/10)" in lines[0]
