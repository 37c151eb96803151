"""HDR clips on the GPU: ssm_frames_accumulate_hdr_fwd (PQ and HLG as the shutter's light) against its float64 yardstick
(ssm_amd.video.accumulate_hdr_host) within the bounds that tests/test_video_hdr_cpu.py derives, black staying black bit for bit, the
entry point's refusals, the two conversions with the BT.2020 table against their host yardsticks bit for bit, and one streamed run
(VideoInterpolator(shutter_light="pq", matrix="bt2020") on a 10-bit 4:2:0 clip) against the chain it stands for, byte for byte.

Shapes of the accumulate tests (planes of H x W, three of them): 5 x 7, one pixel per lane with ragged blocks; 8 x 12, four pixels per
lane; 4 x 260, four pixels per lane and a second workgroup along x (65 lanes).  Each runs as a contiguous tensor and as a view into rows
of W + 9 floats that starts 5 floats in - a row start that is not 16-byte aligned, which puts every shape on the one-pixel path (260
then fills five workgroups along x)."""
import ctypes
import io
import os
import sys
from fractions import Fraction as Fr

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_video_hdr_cpu import B, B_LIGHT, MEAN, NAMES, STD  # noqa: E402
from video_clips import V, synthetic_model  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
POISON = np.uint32(0x7FC0DEAD)
SHAPES = [(5, 7), (8, 12), (4, 260)]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def poisoned(shape):
    return torch.from_numpy(np.full(shape, POISON, np.uint32).view(np.float32)).to(DEV)


def views(h, w, n, strided):
    """(src view [n,3,h,w], acc buffer, acc view [1,3,h,w] into it, the view's region of the buffer), everything poisoned."""
    if strided:
        sbuf, abuf, at = poisoned((n, 3, h + 2, w + 9)), poisoned((1, 3, h + 2, w + 9)), (1, 5)
    else:
        sbuf, abuf, at = poisoned((n, 3, h, w)), poisoned((1, 3, h, w)), (0, 0)
    region = (slice(None), slice(None), slice(at[0], at[0] + h), slice(at[1], at[1] + w))
    src, acc = sbuf[region], abuf[region]
    vec = w % 4 == 0 and all(t.data_ptr() % 16 == 0 and all(s % 4 == 0 for s in t.stride()[:3]) for t in (src, acc))
    assert vec == (w % 4 == 0 and not strided)
    return src, abuf, acc, region


BLACK = ((np.float32(0.0) / np.float32(255.0) - np.float32(MEAN)) / np.float32(STD)).astype(np.float32)


def values(rng, shape):
    """Normalised planes whose coded values are random in [0, 1], with the special ones in the first places of every plane: exact black and
    white, HLG's join and its neighbours, PQ's smallest codes with light, a 10-bit step, values below 0 and above 1; the last pixel of
    every plane is the ingest kernels' black in every frame."""
    m, s = (np.asarray(x, np.float32).reshape(1, 3, 1, 1) for x in (MEAN, STD))
    c = rng.uniform(0.0, 1.0, shape).astype(np.float32)
    half = np.float32(0.5)
    special = [0.0, 1.0, half, np.nextafter(half, np.float32(0)), np.nextafter(half, np.float32(1)), 1e-6, 1 / 1023, -0.25, 1.5, -1e-3, 1.001]
    flat = c.reshape(shape[0], 3, -1)
    for f in range(shape[0]):
        flat[f, :, :len(special)] = np.roll(np.float32(special), f)
    x = ((c - m) / s).astype(np.float32)
    x.reshape(shape[0], 3, -1)[:, :, -1] = BLACK
    return x


@pytest.mark.parametrize("strided", [False, True], ids=["contiguous", "strided"])
@pytest.mark.parametrize("shape", SHAPES, ids=["5x7", "8x12", "4x260"])
@pytest.mark.parametrize("name", NAMES)
def test_kernel_is_within_the_bound_of_the_float64_yardstick(name, shape, strided):
    from ssm_amd import hipbind as hb
    v = V()
    kind, row = v.hdr_light(name)
    rng = np.random.default_rng(17)
    worst = {0: 0.0, 1: 0.0}
    for n in (1, 3):
        for init in (0, 1):
            for encode in (0, 1):
                src, abuf, acc, region = views(*shape, n, strided)
                src.copy_(torch.from_numpy(values(rng, tuple(src.shape))))
                held = 0 if init else 3          # an accumulator that continues holds sums of light of 3 samples already
                start = (rng.uniform(0.0, 1.0, tuple(acc.shape)) * held).astype(np.float32)
                start.reshape(3, -1)[:, -1] = 0.0
                acc.copy_(torch.from_numpy(start))
                scale = np.float32(1.0 / (held + n)) if encode else np.float32(1.0)
                want_buf = abuf.cpu().numpy()
                want = v.accumulate_hdr_host(src.cpu().numpy(), start.astype(np.float64), init, scale, MEAN, STD, name, encode)
                assert hb.frames_accumulate_hdr(src, acc, init, scale, MEAN, STD, kind, row, encode) is acc
                torch.cuda.synchronize()
                got_buf = abuf.cpu().numpy()
                got = got_buf[region]
                d = float(np.abs(got.astype(np.float64) - want).max())
                worst[encode] = max(worst[encode], d)
                print("%s %s n=%d init=%d encode=%d: |kernel - float64| %.3g" % (name, shape, n, init, encode, d))
                assert d <= (B[name] if encode else B_LIGHT[name]), (n, init, encode, d)
                last = got.reshape(3, -1)[:, -1]          # black in every frame, and no light held
                assert np.array_equal(bits(last), bits(BLACK if encode else np.zeros(3, np.float32))), (n, init, encode)
                got_buf[region] = want_buf[region]
                assert np.array_equal(bits(got_buf), bits(want_buf)), "an element outside the region lost its poison bits"
    print("%s %s %s: worst |kernel - float64| %.3g of %.3g (encode = 1), %.3g of %.3g (encode = 0)"
          % (name, shape, "strided" if strided else "contiguous", worst[1], B[name], worst[0], B_LIGHT[name]))


@pytest.mark.parametrize("name", NAMES)
def test_black_stays_black_and_values_at_or_below_it_add_nothing(name):
    from ssm_amd import hipbind as hb
    kind, row = V().hdr_light(name)
    m32, s32 = np.float32(MEAN).reshape(1, 3, 1, 1), np.float32(STD).reshape(1, 3, 1, 1)
    black = BLACK.reshape(1, 3, 1, 1)
    rng = np.random.default_rng(1)
    x = ((rng.uniform(0, 1, (8, 3, 6, 12)).astype(np.float32) - m32) / s32).astype(np.float32)
    x[:, :, :3, :] = black
    x[3, :, 0, :] = (black - np.float32(2.0))[0, :, 0]          # below black in one of the samples
    src, acc = torch.from_numpy(x).to(DEV), poisoned((1, 3, 6, 12))
    for first, count in ((0, 3), (3, 1), (4, 4)):
        hb.frames_accumulate_hdr(src[first:first + count], acc, first == 0, np.float32(0.125) if first == 4 else 1.0, MEAN, STD, kind, row, first == 4)
    got = acc.cpu().numpy()
    assert np.array_equal(bits(got[:, :, :3, :]), bits(np.broadcast_to(black, (1, 3, 3, 12))))
    assert not np.array_equal(bits(got[:, :, 3:, :]), bits(np.broadcast_to(black, (1, 3, 3, 12))))
    held = rng.uniform(0, 5, (1, 3, 6, 12)).astype(np.float32)
    acc.copy_(torch.from_numpy(held))
    below = (np.broadcast_to(black, (5, 3, 6, 12)) - rng.uniform(0, 3, (5, 3, 6, 12)).astype(np.float32)).astype(np.float32)
    below[0] = black[0]
    hb.frames_accumulate_hdr(torch.from_numpy(below).to(DEV), acc, 0, 1.0, MEAN, STD, kind, row, 0)
    assert np.array_equal(bits(acc.cpu().numpy()), bits(held))


def test_refusals_leave_the_accumulator_alone():
    from ssm_amd import hipbind as hb
    lib, v = hb.load(), V()
    src, abuf, acc, _ = views(8, 12, 2, False)
    src.copy_(torch.from_numpy(np.random.default_rng(3).uniform(-2, 2, tuple(src.shape)).astype(np.float32)))
    before, src_before = bits(abuf.cpu().numpy()).copy(), bits(src.cpu().numpy()).copy()
    sv, av, null = hb.view_of(src), hb.view_of(acc), hb.SsmView(None, 0, 0, 0)
    n, _, h, w = src.shape
    f, f3 = ctypes.c_float, lambda *x: (ctypes.c_float * 3)(*x)

    def row(name, **kw):
        names = {"pq": "im2 c1 c2 c3 im1 m1 m2 pad", "hlg": "third kexp cc b twelfth aln2 pad0 pad1"}[name].split()
        return (ctypes.c_float * 8)(*[kw.get(k, float(x)) for k, x in zip(names, v.hdr_light(name)[1])])
    mean, std = f3(*MEAN), f3(*STD)
    still = hb.SsmView(src.data_ptr(), 0, src.stride(1), src.stride(2))
    short_s = hb.SsmView(src.data_ptr(), src.stride(0), src.stride(1), w - 1)
    short_a = hb.SsmView(acc.data_ptr(), acc.stride(0), acc.stride(1), w - 1)
    ok = (sv, av, n, h, w, 1, f(0.5), mean, std, 0, row("pq"), 1)

    def but(**kw):
        names = "src acc n h w init scale mean std kind consts encode".split()
        return tuple(kw.get(k, x) for k, x in zip(names, ok))
    nan, inf = float("nan"), float("inf")
    hlg = dict(kind=1, consts=row("hlg"))
    bad = {"null src": but(src=null), "null acc": but(acc=null), "null mean": but(mean=None), "null std": but(std=None),
           "null consts": but(consts=None), "N = 0": but(n=0), "N = 65536": but(src=still, n=65536), "H = 0": but(h=0), "W = 0": but(w=0),
           "H beyond the grid": but(h=262141), "short src rows": but(src=short_s), "short acc rows": but(acc=short_a),
           "init = 2": but(init=2), "init = -1": but(init=-1), "encode = 2": but(encode=2), "encode = -1": but(encode=-1),
           "scale nan": but(scale=f(nan)), "scale inf": but(scale=f(inf)), "std 0": but(std=f3(0.229, 0.0, 0.225)),
           "std nan": but(std=f3(0.229, 0.224, nan)), "mean inf": but(mean=f3(inf, 0.456, 0.406)),
           "kind = 2": but(kind=2), "kind = -1": but(kind=-1), "kind = -1 hlg": but(kind=-1, consts=row("hlg")),
           "pq m1 = 0": but(consts=row("pq", m1=0.0)), "pq 1/m2 < 0": but(consts=row("pq", im2=-0.0127)), "pq c3 nan": but(consts=row("pq", c3=nan)),
           "pq c2 <= c3": but(consts=row("pq", c2=18.0)), "pq pad inf": but(consts=row("pq", pad=inf)),
           "hlg a ln 2 = 0": but(kind=1, consts=row("hlg", aln2=0.0)), "hlg cc nan": but(kind=1, consts=row("hlg", cc=nan)),
           "hlg 1/12 < 0": but(kind=1, consts=row("hlg", twelfth=-1.0 / 12)),
           "acc among the frames": but(acc=hb.view_of(src[1:2])), "acc among the frames, hlg": but(acc=hb.view_of(src[1:2]), **hlg)}
    for what, args in bad.items():
        rc = lib.ssm_frames_accumulate_hdr_fwd(*args, hb.stream_ptr())
        assert rc == -1, what
        assert b"frames_accumulate_hdr" in lib.ssm_last_error_string(), what
    torch.cuda.synchronize()
    assert np.array_equal(bits(abuf.cpu().numpy()), before), "a refused call wrote the accumulator"
    assert np.array_equal(bits(src.cpu().numpy()), src_before), "a refused call wrote the frames"
    for what, named in (("std 0", b"std 0"), ("pq m1 = 0", b"m1=0"), ("pq c2 <= c3", b"c2=18"), ("hlg a ln 2 = 0", b"a ln 2=0"),
                        ("encode = 2", b"encode must be 0 or 1 (got 2)"), ("init = 2", b"init must be 0 or 1 (got 2)"),
                        ("scale nan", b"scale must be finite"), ("short acc rows", b"shorter than W"), ("null consts", b"null pointer"),
                        ("N = 0", b"bad sizes"), ("kind = 2", b"kind 2 not in"), ("kind = -1", b"kind -1 not in"),
                        ("acc among the frames", b"overlap")):
        assert lib.ssm_frames_accumulate_hdr_fwd(*bad[what], hb.stream_ptr()) == -1 and named in lib.ssm_last_error_string(), what
    with pytest.raises(RuntimeError, match="overlap"):
        hb.frames_accumulate_hdr(src, src[1:2], 1, 1.0, MEAN, STD, *v.hdr_light("hlg"), 0)
    with pytest.raises(AssertionError, match="8 floats"):
        hb.frames_accumulate_hdr(src, acc, 1, 1.0, MEAN, STD, 0, v.hdr_light("pq")[1][:7], 0)
    torch.cuda.synchronize()
    assert np.array_equal(bits(abuf.cpu().numpy()), before)


# ---- BT.2020 through the conversion kernels --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("crange", [0, 1])
@pytest.mark.parametrize("layout", [0, 1, 2, 3])
@pytest.mark.parametrize("nbits", [8, 10])
def test_bt2020_kernels_equal_their_yardsticks(nbits, layout, crange):
    v = V()
    for n, (h, w) in enumerate([(6, 8), (7, 10)]):
        rng = np.random.RandomState(1000 * layout + 100 * nbits + 10 * crange + n)
        fb = v.frame_bytes(h, w, layout, nbits)
        if nbits == 8:
            payload = rng.randint(0, 256, size=(2, fb)).astype(np.uint8)
        else:
            payload = rng.randint(0, 1 << nbits, size=(2, fb // 2)).astype("<u2").view(np.uint8)
        for pbn in (True, False):
            got = v.frames_from_yuv(torch.from_numpy(payload).to(DEV), h, w, layout, v.BT2020, crange, None, pbn, bits=nbits).cpu().numpy()
            want = v.yuv_to_frames_host(payload, h, w, layout, v.BT2020, crange, pad_before_norm=pbn, bits=nbits)
            np.testing.assert_array_equal(bits(got), bits(want))
        other = v.yuv_to_frames_host(payload, h, w, layout, v.BT709, crange, bits=nbits)
        assert not np.array_equal(v.yuv_to_frames_host(payload, h, w, layout, v.BT2020, crange, bits=nbits), other), "another matrix, another picture"
        hp, wp = want.shape[2:]
        x = rng.uniform(-2.3, 2.8, size=(2, 3, hp, wp)).astype(np.float32)
        got = v.frames_to_yuv(torch.from_numpy(x).to(DEV), h, w, layout, v.BT2020, crange, bits=nbits).cpu().numpy()
        np.testing.assert_array_equal(got, v.frames_to_yuv_host(x, h, w, layout, v.BT2020, crange, bits=nbits))


# ---- the streamed loop ---------------------------------------------------------------------------------------------------------------------
H = W = 64
N = 5
A = dict(target_rate=(24, 1), shutter="1/2", shutter_samples=4)          # 60 -> 24: step 5/2, two outputs from five frames
STEP, SIGMA, S = Fr(5, 2), Fr(1, 2), 4


def run_stream(m, cfg, payloads, **kw):
    v = V()
    buf = io.BytesIO()
    with v.Y4MWriter(buf, W, H, rate=(60, 1), aspect=(1, 1), chroma="420p10", extended=True) as wr:
        for p in payloads:
            wr.write_frame(p)
    r = v.Y4MReader(io.BytesIO(buf.getvalue()), extended=True)
    sink = io.BytesIO()
    wr = v.Y4MWriter.like(sink, r, rate=(24, 1))
    count = v.VideoInterpolator(m, cfg, **kw).run(r, wr)
    out = v.Y4MReader(io.BytesIO(sink.getvalue()), extended=True)
    frames, one = [], np.empty(out.frame_bytes, np.uint8)
    while out.read_frame_into(one):
        frames.append(one.copy())
    assert len(frames) == count and out.rate == (24, 1)
    return np.stack(frames)


def test_stream_is_the_chain_it_stands_for():
    from ssm_amd import hipbind as hb
    from ssm_amd.weights import synthetic_frames_u8
    v = V()
    cfg, m = synthetic_model(DEV)
    rgb = synthetic_frames_u8(N, H, W, seed=5).numpy().astype(np.float32) / np.float32(255.0)
    x = (rgb - np.float32(MEAN)[None, :, None, None]) / np.float32(STD)[None, :, None, None]
    payloads = v.frames_to_yuv_host(x, H, W, v.CENTRED, v.BT2020, v.LIMITED, bits=10)
    got = run_stream(m, cfg, payloads, n_streams=2, shutter_light="pq", matrix=v.MATRICES["bt2020"], **A)
    tl = v.Timeline(STEP, shutter=SIGMA, samples=S)
    assert got.shape == (2, payloads.shape[1]) and tl.n_outputs(N) == 2
    # ingest, the pairs at their sample times, the accumulate calls in time order, egress: the same kernels, call for call
    dev = torch.from_numpy(payloads).to(DEV)
    coding = dict(bits=10)
    planes = v.frames_from_yuv(dev, H, W, v.CENTRED, v.BT2020, v.LIMITED, cfg, True, **coding)
    made = {}
    for i in range(N - 1):
        ts = [float(v.Timeline.t32(t)) for t, _, _ in tl.times(i)]
        if ts:
            pair = v.frames_from_yuv(dev[i:i + 2], H, W, v.CENTRED, v.BT2020, v.LIMITED, cfg, True, **coding)
            made[i] = m.interpolate(pair[None], ts + [ts[-1]] * (tl.slots - len(ts)))
    kind, row = v.hdr_light("pq")
    want = []
    for smp in tl.outputs(N):
        acc = poisoned((1,) + tuple(planes.shape[1:]))
        for j, (i, t) in enumerate(smp):
            frame = planes[i] if t == 0 else made[i][[x for x, _, _ in tl.times(i)].index(t)]
            hb.frames_accumulate_hdr(frame[None], acc, 1 if j == 0 else 0, np.float32(1.0 / S) if j == S - 1 else 1.0, MEAN, STD, kind, row,
                                     1 if j == S - 1 else 0)
        want.append(v.frames_to_yuv(acc, H, W, v.CENTRED, v.BT2020, v.LIMITED, cfg, **coding).cpu().numpy()[0])
    want = np.stack(want)
    assert np.array_equal(got, want), int((got != want).sum())
    coded = run_stream(m, cfg, payloads, n_streams=2, shutter_light="coded", matrix=v.MATRICES["bt2020"], **A)
    assert coded.shape == got.shape and not np.array_equal(coded, got), "the mean of light is another picture than the mean of the codes"
    other = run_stream(m, cfg, payloads, n_streams=2, shutter_light="pq", **A)
    assert not np.array_equal(other, got), "BT.601, the default of a 64-row clip, is another matrix"
