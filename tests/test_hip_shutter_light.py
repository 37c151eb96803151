"""The shutter in linear light on the GPU: ssm_frames_accumulate_light_fwd against its float64 yardstick
(ssm_amd.video.accumulate_light_host) within the bound that tests/test_video_light_cpu.py derives, its two exact properties, its
refusals, and the streamed loop (VideoInterpolator(shutter_light=), scripts/interpolate_video.py --shutter_light) against the chain it
stands for: ingest -> FullModel.interpolate of every running pair at its sample times, padded to `slots` (tests/test_hip_shutter.py says
why) -> accumulate_light_host in float64 over each output's samples in time order -> frames_to_yuv_host.  The clip is the 9-frame 64 x 48
clip at 60:1 of tests/test_hip_shutter.py, built the same way."""
import functools
import os
import sys
from fractions import Fraction as Fr

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import video_clips  # noqa: E402
from test_video_light_cpu import B, B_LIGHT, CURVES, MEAN, STD, bound  # noqa: E402
from video_clips import V, clip_payloads, read_clip  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
H, W, N = 40, 48, 9          # canvas 64 x 64
clip_file = functools.partial(video_clips.clip_file, rate=(60, 1))
stream = functools.partial(video_clips.stream, rate=(60, 1))
POISON = np.uint32(0x7FC0DEAD)
NORMS = {"config": (MEAN, STD), "narrow": ((0.5, 0.25, 0.625), (0.125, 0.0625, 0.03125))}          # the second: std well below 1


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def poisoned(shape):
    return torch.from_numpy(np.full(shape, POISON, np.uint32).view(np.float32)).to(DEV)


# ---- the kernel ----------------------------------------------------------------------------------------------------------------------
def views(name, n):
    """(src view [n,3,h,w], acc buffer, acc view [1,3,h,w] into it, the view's region of the buffer), everything poisoned."""
    if name == "5x7":             # an odd offset of a 12 x 16 canvas: one element per lane, a partial row block and column block
        sbuf, abuf, at, (h, w) = poisoned((n, 3, 12, 16)), poisoned((1, 3, 12, 16)), (3, 5), (5, 7)
    elif name == "6x12":          # 16-byte aligned rows, strides of multiples of 4: four pixels per lane
        sbuf, abuf, at, (h, w) = poisoned((n, 3, 8, 20)), poisoned((1, 3, 8, 20)), (1, 4), (6, 12)
    else:                         # "6x12 strided": W = 12 at an offset of 5 floats in rows of 21: one element per lane
        sbuf, abuf, at, (h, w) = poisoned((n, 3, 8, 21)), poisoned((1, 3, 8, 21)), (1, 5), (6, 12)
    region = (slice(None), slice(None), slice(at[0], at[0] + h), slice(at[1], at[1] + w))
    src, acc = sbuf[region], abuf[region]
    vec = w % 4 == 0 and all(t.data_ptr() % 16 == 0 and all(s % 4 == 0 for s in t.stride()[:3]) for t in (src, acc))
    assert vec == (name == "6x12")
    return src, abuf, acc, region


def values(rng, shape, mean, std, row):
    """Normalised planes whose coded values are random in [0, 1], with the special ones in the first places of every plane: the coded
    black and white, thr and its neighbours one ulp either side, 1e-6, values below 0 and above 1."""
    m, s = (np.asarray(x, np.float32).reshape(1, 3, 1, 1) for x in (mean, std))
    c = rng.uniform(0.0, 1.0, shape).astype(np.float32)
    thr = np.float32(row[0])
    special = [0.0, 1.0, thr, np.nextafter(thr, np.float32(-1)), np.nextafter(thr, np.float32(2)), 1e-6, -0.25, 1.5, -1e-3, 1.001]
    flat = c.reshape(shape[0], 3, -1)
    for f in range(shape[0]):
        flat[f, :, :len(special)] = np.roll(np.float32(special), f)          # every frame meets them in other places
    x = ((c - m) / s).astype(np.float32)
    black = ((np.float32(0.0) / np.float32(255.0) - m) / s).astype(np.float32)
    x.reshape(shape[0], 3, -1)[:, :, -1] = black[:, :, 0, 0]                # the last pixel of every plane is black in every frame
    return x


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("norm", sorted(NORMS))
@pytest.mark.parametrize("name", ["5x7", "6x12", "6x12 strided"])
def test_kernel_is_within_the_bound_of_the_float64_yardstick(name, norm, curve):
    from ssm_amd import hipbind as hb
    v = V()
    mean, std = NORMS[norm]
    row = v.light_curve(curve)
    rng = np.random.default_rng(17)
    bar = bound(mean, std)
    assert norm != "config" or bar <= B
    worst = {0: 0.0, 1: 0.0}
    for n in (1, 2, 5):
        for init in (0, 1):
            for encode in (0, 1):
                src, abuf, acc, region = views(name, n)
                src.copy_(torch.from_numpy(values(rng, tuple(src.shape), mean, std, row)))
                held = 0 if init else 3          # samples an accumulator that continues holds already: sums of light in [0, 3]
                start = (rng.uniform(0.0, 1.0, tuple(acc.shape)) * held).astype(np.float32)
                start.reshape(3, -1)[:, -1] = 0.0
                acc.copy_(torch.from_numpy(start))
                scale = np.float32(1.0 / (held + n)) if encode else np.float32(1.0)
                want_buf = abuf.cpu().numpy()
                want = v.accumulate_light_host(src.cpu().numpy(), start.astype(np.float64), init, scale, mean, std, row, encode)
                assert hb.frames_accumulate_light(src, acc, init, scale, mean, std, row, encode) is acc
                torch.cuda.synchronize()
                got_buf = abuf.cpu().numpy()
                got = got_buf[region]
                d = float(np.abs(got.astype(np.float64) - want).max())
                worst[encode] = max(worst[encode], d)
                assert d <= (bar if encode else B_LIGHT), (n, init, encode, d)
                # the two exact properties, on the plane's last pixel: black in every frame (and no light held)
                m32, s32 = np.float32(mean), np.float32(std)
                black = (np.float32(0.0) / np.float32(255.0) - m32) / s32
                last = got.reshape(3, -1)[:, -1]
                assert np.array_equal(bits(last), bits(black if encode else np.zeros(3, np.float32))), (n, init, encode)
                got_buf[region] = want_buf[region]
                assert np.array_equal(bits(got_buf), bits(want_buf)), "an element outside the region lost its poison bits"
    print("%s %s %s: worst |kernel - float64| %.3g of %.3g (encode = 1), %.3g of %.3g (encode = 0)"
          % (name, norm, curve, worst[1], bar, worst[0], B_LIGHT))


@pytest.mark.parametrize("curve", CURVES)
def test_black_stays_black_and_values_at_or_below_it_add_nothing(curve):
    """A region that is black in all S = 8 samples comes back as the ingest kernels' black, bit for bit, through a chain of calls; and
    frames of coded values <= 0 leave a sum of light exactly as it was."""
    from ssm_amd import hipbind as hb
    v = V()
    row = v.light_curve(curve)
    m32, s32 = np.float32(MEAN).reshape(1, 3, 1, 1), np.float32(STD).reshape(1, 3, 1, 1)
    black = ((np.float32(0.0) / np.float32(255.0) - m32) / s32).astype(np.float32)
    rng = np.random.default_rng(1)
    x = ((rng.uniform(0, 1, (8, 3, 6, 12)).astype(np.float32) - m32) / s32).astype(np.float32)
    x[:, :, :3, :] = black
    x[3, :, 0, :] = (black - np.float32(2.0))[0, :, 0]          # below black in one of the samples
    src, acc = torch.from_numpy(x).to(DEV), poisoned((1, 3, 6, 12))
    for first, count in ((0, 3), (3, 1), (4, 4)):
        hb.frames_accumulate_light(src[first:first + count], acc, first == 0, np.float32(0.125) if first == 4 else 1.0, MEAN, STD, row, first == 4)
    got = acc.cpu().numpy()
    assert np.array_equal(bits(got[:, :, :3, :]), bits(np.broadcast_to(black, (1, 3, 3, 12))))
    assert not np.array_equal(bits(got[:, :, 3:, :]), bits(np.broadcast_to(black, (1, 3, 3, 12))))
    held = rng.uniform(0, 5, (1, 3, 6, 12)).astype(np.float32)
    acc.copy_(torch.from_numpy(held))
    below = (np.broadcast_to(black, (5, 3, 6, 12)) - rng.uniform(0, 3, (5, 3, 6, 12)).astype(np.float32)).astype(np.float32)
    below[0] = black[0]
    hb.frames_accumulate_light(torch.from_numpy(below).to(DEV), acc, 0, 1.0, MEAN, STD, row, 0)
    assert np.array_equal(bits(acc.cpu().numpy()), bits(held))


def test_refusals_leave_the_accumulator_alone():
    import ctypes
    from ssm_amd import hipbind as hb
    lib, v = hb.load(), V()
    src, abuf, acc, _ = views("6x12", 2)
    src.copy_(torch.from_numpy(np.random.default_rng(3).uniform(-2, 2, tuple(src.shape)).astype(np.float32)))
    before, src_before = bits(abuf.cpu().numpy()).copy(), bits(src.cpu().numpy()).copy()
    sv, av, null = hb.view_of(src), hb.view_of(acc), hb.SsmView(None, 0, 0, 0)
    n, _, h, w = src.shape
    f, f3 = ctypes.c_float, lambda *x: (ctypes.c_float * 3)(*x)
    row = lambda **kw: (ctypes.c_float * 9)(*[kw.get(k, float(x)) for k, x in zip("thr islope a i1a g lthr slope a1 ig".split(), v.light_curve("srgb"))])
    mean, std, srgb = f3(*MEAN), f3(*STD), row()
    still = hb.SsmView(src.data_ptr(), 0, src.stride(1), src.stride(2))          # every frame the first one: no size reaches past the buffer
    short_s = hb.SsmView(src.data_ptr(), src.stride(0), src.stride(1), w - 1)
    short_a = hb.SsmView(acc.data_ptr(), acc.stride(0), acc.stride(1), w - 1)
    ok = (sv, av, n, h, w, 1, f(0.5), mean, std, srgb, 1)

    def but(**kw):
        names = "src acc n h w init scale mean std curve encode".split()
        return tuple(kw.get(k, x) for k, x in zip(names, ok))
    nan, inf = float("nan"), float("inf")
    bad = {"null src": but(src=null), "null acc": but(acc=null), "null mean": but(mean=None), "null std": but(std=None),
           "null curve": but(curve=None), "N = 0": but(n=0), "N = -1": but(n=-1), "N = 65536": but(src=still, n=65536), "H = 0": but(h=0),
           "W = 0": but(w=0), "H beyond the grid": but(h=262141), "short src rows": but(src=short_s), "short acc rows": but(acc=short_a),
           "init = 2": but(init=2), "init = -1": but(init=-1), "encode = 2": but(encode=2), "encode = -1": but(encode=-1),
           "scale nan": but(scale=f(nan)), "scale inf": but(scale=f(inf)), "std 0": but(std=f3(0.229, 0.0, 0.225)),
           "std nan": but(std=f3(0.229, 0.224, nan)), "mean inf": but(mean=f3(inf, 0.456, 0.406)), "g = 0": but(curve=row(g=0.0)),
           "g < 0": but(curve=row(g=-2.4)), "g nan": but(curve=row(g=nan)), "slope = 0": but(curve=row(slope=0.0)),
           "slope < 0": but(curve=row(slope=-12.92)), "acc among the frames": but(acc=hb.view_of(src[1:2]))}
    for what, args in bad.items():
        rc = lib.ssm_frames_accumulate_light_fwd(*args, hb.stream_ptr())
        assert rc == -1, what
        assert b"frames_accumulate_light" in lib.ssm_last_error_string(), what
    torch.cuda.synchronize()
    assert np.array_equal(bits(abuf.cpu().numpy()), before), "a refused call wrote the accumulator"
    assert np.array_equal(bits(src.cpu().numpy()), src_before), "a refused call wrote the frames"
    for what, named in (("std 0", b"std 0"), ("g = 0", b"g=0"), ("slope < 0", b"slope=-12.92"), ("encode = 2", b"encode must be 0 or 1 (got 2)"),
                        ("init = 2", b"init must be 0 or 1 (got 2)"), ("scale nan", b"scale must be finite"), ("short acc rows", b"shorter than W"),
                        ("null curve", b"null pointer"), ("N = 0", b"bad sizes")):
        assert lib.ssm_frames_accumulate_light_fwd(*bad[what], hb.stream_ptr()) == -1 and named in lib.ssm_last_error_string(), what
    with pytest.raises(RuntimeError, match="overlap"):
        hb.frames_accumulate_light(src, src[1:2], 1, 1.0, MEAN, STD, v.light_curve("srgb"), 0)
    with pytest.raises(AssertionError, match="9 floats"):
        hb.frames_accumulate_light(src, acc, 1, 1.0, MEAN, STD, v.light_curve("srgb")[:8], 0)


# ---- the streamed loop ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    from models.superslomo_r import FullModel
    from ssm_amd.config import load_config, synthetic_weight_overrides
    from ssm_amd.weights import synthetic_state_dict
    cfg = load_config("superslomo_original.ini", synthetic_weight_overrides())
    m = FullModel(cfg)
    m.stage1_model.load_state_dict(synthetic_state_dict(1))
    m.stage2_model.load_state_dict(synthetic_state_dict(2))
    return cfg, m.to(DEV).eval()


A = dict(target_rate=(24, 1), shutter=Fr(1, 2), shutter_samples=4)          # 60 -> 24: step 5/2
STEP, SIGMA, S = Fr(5, 2), Fr(1, 2), 4


def codes_before_rounding(x, h, w, matrix, crange):
    """The egress of normalised planes [N,3,Hp,Wp] in float64 up to the rounding: [N, frame_bytes] code values, 4:2:0 centred."""
    v = V()
    k = v.yuv_table()[matrix, crange].astype(np.float64)
    kr, kg, kb, cbs, crs, iys, ics, yoff, coff = k[0], k[1], k[2], k[7], k[8], k[11], k[12], k[13], k[14]
    n, _, hp, wp = x.shape
    top, left = (hp - h) // 2, (wp - w) // 2
    r, g, b = ((x[:, p, top:top + h, left:left + w].astype(np.float64) * np.float64(np.float32(STD[p])) + np.float64(np.float32(MEAN[p]))) * 255.0
               for p in range(3))
    yf = kr * r + kg * g + kb * b
    assert h % 2 == 0 and w % 2 == 0
    sub = lambda c: c.reshape(n, h // 2, 2, w // 2, 2).mean(axis=(2, 4))
    planes = [yf * iys + yoff, sub((b - yf) * cbs) * ics + coff, sub((r - yf) * crs) * ics + coff]
    return np.concatenate([p.reshape(n, -1) for p in planes], axis=1)


@pytest.fixture(scope="module")
def chain(model):
    """(payloads, the host chain's output, the samples a legitimate error may flip), computed once."""
    cfg, m = model
    v = V()
    payloads = clip_payloads(N, H, W, 0)
    tl = v.Timeline(STEP, shutter=SIGMA, samples=S)
    dev = torch.from_numpy(payloads).to(DEV)
    matrix, crange = v.default_matrix(H), v.LIMITED
    planes = v.frames_from_yuv(dev, H, W, 0, matrix, crange, cfg, True).cpu().numpy()
    made = {}
    for i in range(N - 1):
        ts = [float(v.Timeline.t32(t)) for t, _, _ in tl.times(i)]
        if ts:
            x = v.frames_from_yuv(dev[i:i + 2], H, W, 0, matrix, crange, cfg, True)
            made[i] = m.interpolate(x[None], ts + [ts[-1]] * (tl.slots - len(ts))).cpu().numpy()
    row, scale, accs = v.light_curve("srgb"), np.float32(1.0 / S), []
    for smp in tl.outputs(N):
        acc = np.full((1,) + planes.shape[1:], np.nan, np.float64)
        for j, (i, t) in enumerate(smp):
            frame = planes[i] if t == 0 else made[i][[x for x, _, _ in tl.times(i)].index(t)]
            v.accumulate_light_host(frame[None], acc, 1 if j == 0 else 0, scale if j == S - 1 else 1.0, MEAN, STD, row, 1 if j == S - 1 else 0)
        accs.append(acc[0].astype(np.float32))
    accs = np.stack(accs)
    want = v.frames_to_yuv_host(accs, H, W, 0, matrix, crange)
    pre = codes_before_rounding(accs, H, W, matrix, crange)
    assert np.abs(np.clip(np.rint(pre), 16, 240) - want).max() <= 1, "the float64 egress is the yardstick's up to its own ties"
    width = B * 255 * max(STD)          # carried through the luma and chroma weights, whose absolute sums are <= 1
    may_flip = np.abs(pre - np.floor(pre) - 0.5) <= width
    share = may_flip.mean()
    print("samples within %.3g of a tie in the float64 chain: %d of %d (%.3f %%)" % (width, may_flip.sum(), may_flip.size, 100 * share))
    assert share < 0.02, "a condition on the clip: change its seed"
    return payloads, want, may_flip


@pytest.mark.parametrize("pairs", [1, 2])
def test_stream_against_the_float64_chain(model, chain, pairs):
    cfg, m = model
    payloads, want, may_flip = chain
    hdr, got = stream(m, cfg, payloads, H, W, n_streams=2, pairs_per_batch=pairs, shutter_light="srgb", **A)
    assert got.shape == want.shape and got.shape[0] == 3 and hdr.rate == (24, 1)
    diff = np.abs(got.astype(int) - want.astype(int))
    print("%d pair(s) per pass: %d codes differ from the chain, %d of them outside the set a legitimate error may flip, by %d at most"
          % (pairs, int((diff != 0).sum()), int((diff != 0)[~may_flip].sum()), int(diff.max())))
    assert diff.max() <= 1
    assert not (diff != 0)[~may_flip].any()
    _, coded = stream(m, cfg, payloads, H, W, n_streams=2, pairs_per_batch=pairs, **A)
    assert not np.array_equal(coded, got), "the mean of light is another picture than the mean of the codes"


def test_coded_is_the_run_without_the_argument(model):
    cfg, m = model
    payloads = clip_payloads(N, H, W, 0)
    _, plain = stream(m, cfg, payloads, H, W, n_streams=2, **A)
    _, coded = stream(m, cfg, payloads, H, W, n_streams=2, shutter_light="coded", **A)
    assert np.array_equal(coded, plain)


def test_cli_round_trip(model, tmp_path, caplog):
    import logging
    import interpolate_video
    cfg, m = model
    v = V()
    payloads = clip_payloads(N, H, W, 0)
    src, dst, ini, logf = (str(tmp_path / x) for x in ("in.y4m", "out.y4m", "cfg.ini", "log.txt"))
    with open(src, "wb") as f:
        f.write(clip_file(payloads, H, W).getvalue())
    with open(ini, "w") as f:
        cfg.write(f)
    argv = ["-c", ini, "--expt", "t", "--log", logf, "--input", src, "--output", dst, "--fps", "24", "--shutter", "180", "--shutter_samples", "4",
            "--shutter_light", "bt709"]
    count = v.Timeline(STEP, shutter=SIGMA, samples=S).n_outputs(N)
    with caplog.at_level(logging.INFO):
        assert interpolate_video.main(argv, model=m) == count == 3
    seen = caplog.messages
    hdr, got = read_clip(dst)
    assert got.shape[0] == count and hdr.rate == (24, 1) and (hdr.width, hdr.height) == (W, H)
    assert any("shutter:" in line and "light (bt709)" in line for line in seen), seen
