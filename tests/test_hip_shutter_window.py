"""The shutter windows on the GPU: ssm_frames_accumulate_weighted_fwd bit for bit against its numpy yardstick
(ssm_amd.video.accumulate_host(..., weights=)) on the three layouts of tests/test_hip_shutter.py, its light and HDR siblings within the
bounds that tests/test_video_window_cpu.py derives, on the frames of tests/test_hip_shutter_light.py and tests/test_hip_video_hdr.py,
the refusals, and the streamed loop (VideoInterpolator(shutter_window=), scripts/interpolate_video.py --shutter_window) byte for byte
against the composition it stands for: tests/test_hip_shutter.py's expected_stream with the window's weights and scale in place of 1 / S."""
import ctypes
import functools
import os
import sys
from fractions import Fraction as Fr

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_hip_shutter_light as light_gpu  # noqa: E402
import test_hip_video_hdr as hdr_gpu  # noqa: E402
import video_clips  # noqa: E402
from test_hip_shutter import case, poisoned  # noqa: E402
from test_video_window_cpu import B_W, B_W_LIGHT, MEAN, PSI, PSI_LIGHT, STD, bound_w, sum_bound  # noqa: E402
from video_clips import V, clip_payloads, read_clip  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
H, W, N = 40, 48, 9          # canvas 64 x 64
clip_file = functools.partial(video_clips.clip_file, rate=(60, 1))
stream = functools.partial(video_clips.stream, rate=(60, 1))
POISON = np.uint32(0x7FC0DEAD)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- the coded kernel ----------------------------------------------------------------------------------------------------------------
def weight_sets(n, rng):
    """(weights, scale) for a call over n frames: ones, the triangle, hann with its scale, one random set in [0, 1) with scale 0.125."""
    v = V()
    return {"ones": (np.ones(n, np.float32), np.float32(1.0 / 3.0)), "triangle": (v.shutter_window("triangle", n)[0], np.float32(1.0)),
            "hann": v.shutter_window("hann", n), "random": (rng.uniform(0.0, 1.0, n).astype(np.float32), np.float32(0.125))}


@pytest.mark.parametrize("name", ["odd", "aligned", "strided"])
def test_weighted_accumulate_is_bit_equal_to_the_yardstick(name):
    from ssm_amd import hipbind as hb
    v = V()
    rng = np.random.default_rng(11)
    for n in (1, 2, 5, 7):          # 5 and 7 leave the unroll by 4 a remainder
        for init in (0, 1):
            for what, (w, scale) in weight_sets(n, rng).items():
                src, abuf, acc = case(name, n, rng)
                want_buf = abuf.cpu().numpy()
                region = tuple(slice(o, o + s) for o, s in zip((0, 0) + ((3, 5) if name == "odd" else (1, 4)), acc.shape))
                want = v.accumulate_host(src.cpu().numpy(), np.ascontiguousarray(want_buf[region]), init, scale, weights=w)
                want_buf[region] = want
                assert hb.frames_accumulate(src, acc, init, scale, weights=w) is acc
                torch.cuda.synchronize()
                got_buf = abuf.cpu().numpy()
                assert np.array_equal(bits(got_buf[region]), bits(want)), (n, init, what, int((bits(got_buf[region]) != bits(want)).sum()))
                assert np.array_equal(bits(got_buf), bits(want_buf)), "an element outside the region lost its poison bits"
                assert int((bits(got_buf) == POISON).sum()) == got_buf.size - acc.numel()


@pytest.mark.parametrize("name", ["odd", "aligned", "strided"])
def test_ones_equal_the_unweighted_kernel_and_pieces_equal_the_one_call(name):
    from ssm_amd import hipbind as hb
    v = V()
    rng = np.random.default_rng(5)
    for init in (0, 1):
        src, abuf, acc = case(name, 7, rng)
        start = acc.clone()
        plain = hb.frames_accumulate(src, acc, init, np.float32(1.0 / 7.0)).clone()
        acc.copy_(start)
        ones = hb.frames_accumulate(src, acc, init, np.float32(1.0 / 7.0), weights=np.ones(7, np.float32)).clone()
        assert np.array_equal(bits(ones.cpu().numpy()), bits(plain.cpu().numpy())), "1 * x is x"
        w, scale = v.shutter_window("hann", 7)
        acc.copy_(start)
        one = hb.frames_accumulate(src, acc, init, scale, weights=w).clone()
        acc.copy_(start)
        hb.frames_accumulate(src[:3], acc, init, 1.0, weights=w[:3])
        hb.frames_accumulate(src[3:], acc, 0, scale, weights=w[3:])
        assert np.array_equal(bits(acc.cpu().numpy()), bits(one.cpu().numpy())), "3 + 4 frames: the same additions in the same order"
        assert not np.array_equal(bits(one.cpu().numpy()), bits(plain.cpu().numpy()))


# ---- the kernels in light ------------------------------------------------------------------------------------------------------------
BLACK = hdr_gpu.BLACK


def _light_case(light, window, init, encode, rng, shape):
    """One weighted call of N = 5 frames in the light `light`: the last five samples of an S = 8 window onto an accumulator that holds
    the first three (init = 0), or a whole S = 5 window (init = 1).  Returns (worst distance, its bound)."""
    from ssm_amd import hipbind as hb
    v = V()
    n = 5
    hdr = light in hdr_gpu.NAMES
    if init:
        w, scale = v.shutter_window(window, n)
        held = 0.0
    else:
        full, scale = v.shutter_window(window, 8)
        w, held = full[3:], float(full[:3].astype(np.float64).sum())
    if hdr:
        src, abuf, acc, region = hdr_gpu.views(*shape, n, shape[1] % 4 != 0)
        src.copy_(torch.from_numpy(hdr_gpu.values(rng, tuple(src.shape))))
        kind, row = v.hdr_light(light)
    else:
        src, abuf, acc, region = light_gpu.views(shape, n)
        row = v.light_curve(light)
        src.copy_(torch.from_numpy(light_gpu.values(rng, tuple(src.shape), MEAN, STD, row)))
    start = (rng.uniform(0.0, 1.0, tuple(acc.shape)) * held).astype(np.float32)          # sums of weighted light of the first three samples
    start.reshape(3, -1)[:, -1] = 0.0
    acc.copy_(torch.from_numpy(start))
    scale = scale if encode else np.float32(1.0)
    want_buf = abuf.cpu().numpy()
    if hdr:
        want = v.accumulate_hdr_host(src.cpu().numpy(), start.astype(np.float64), init, scale, MEAN, STD, light, encode, weights=w)
        assert hb.frames_accumulate_hdr(src, acc, init, scale, MEAN, STD, kind, row, encode, weights=w) is acc
    else:
        want = v.accumulate_light_host(src.cpu().numpy(), start.astype(np.float64), init, scale, MEAN, STD, row, encode, weights=w)
        assert hb.frames_accumulate_light(src, acc, init, scale, MEAN, STD, row, encode, weights=w) is acc
    torch.cuda.synchronize()
    got_buf = abuf.cpu().numpy()
    got = got_buf[region]
    d = float(np.abs(got.astype(np.float64) - want).max())
    if encode:
        bar = B_W[light] if hdr else bound_w(MEAN, STD)
    else:
        bar = sum_bound(w, held, 1.0, PSI[light] if hdr else PSI_LIGHT, init=bool(init))
    last = got.reshape(3, -1)[:, -1]          # black in every frame, and no light held: black stays bit-identical black
    assert np.array_equal(bits(last), bits(BLACK if encode else np.zeros(3, np.float32))), (light, window, init, encode)
    got_buf[region] = want_buf[region]
    assert np.array_equal(bits(got_buf), bits(want_buf)), "an element outside the region lost its poison bits"
    return d, bar


@pytest.mark.parametrize("window", ["triangle", "hann"])
@pytest.mark.parametrize("light", ["srgb", "pq", "hlg"])
def test_kernels_in_light_are_within_the_derived_bounds(light, window):
    assert bound_w(MEAN, STD) <= B_W_LIGHT
    rng = np.random.default_rng(17)
    shapes = [(5, 7), (8, 12)] if light in hdr_gpu.NAMES else ["5x7", "6x12"]          # one pixel per lane; four
    worst = {0: (0.0, 0.0), 1: (0.0, 0.0)}
    for shape in shapes:
        for init in (0, 1):
            for encode in (0, 1):
                d, bar = _light_case(light, window, init, encode, rng, shape)
                print("%s %s %s init=%d encode=%d: |kernel - float64| %.3g of %.3g" % (light, window, shape, init, encode, d, bar))
                assert d <= bar, (shape, init, encode, d, bar)
                worst[encode] = max(worst[encode], (d / bar, d))
    print("%s %s: worst |kernel - float64| %.3g (%.2f of its bound) encoded, %.3g (%.2f of its bound) in light"
          % (light, window, worst[1][1], worst[1][0], worst[0][1], worst[0][0]))


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_accumulator_and_the_frames_alone():
    from ssm_amd import hipbind as hb
    lib, v = hb.load(), V()
    rng = np.random.default_rng(3)
    src, abuf, acc = case("aligned", 2, rng)
    before, src_before = bits(abuf.cpu().numpy()).copy(), bits(src.cpu().numpy()).copy()
    sv, av = hb.view_of(src), hb.view_of(acc)
    n, c, h, w = src.shape
    still = hb.SsmView(src.data_ptr(), 0, src.stride(1), src.stride(2))          # every frame the first one: no size reaches past the buffer
    f, fs = ctypes.c_float, lambda *x: (ctypes.c_float * len(x))(*x)
    nan, inf = float("nan"), float("inf")
    ok2, ok65 = fs(1.0, 3.0), fs(*([1.0] * 65))
    mean, std = fs(*MEAN), fs(*STD)
    srgb = fs(*[float(x) for x in v.light_curve("srgb")])
    kind, pq = v.hdr_light("pq")
    pq = fs(*[float(x) for x in pq])
    entries = {
        "ssm_frames_accumulate_weighted_fwd": lambda s, cnt, wt: (s, av, cnt, c, h, w, 1, f(0.5), wt),
        "ssm_frames_accumulate_light_weighted_fwd": lambda s, cnt, wt: (s, av, cnt, h, w, 1, f(0.5), wt, mean, std, srgb, 1),
        "ssm_frames_accumulate_hdr_weighted_fwd": lambda s, cnt, wt: (s, av, cnt, h, w, 1, f(0.5), wt, mean, std, kind, pq, 1),
    }
    for entry, args in entries.items():
        bad = {"null weights": args(sv, n, None), "N = 65": args(still, 65, ok65), "a NaN weight": args(sv, n, fs(1.0, nan)),
               "an infinite weight": args(sv, n, fs(-inf, 1.0)), "N = 0": args(sv, 0, ok2), "null src": args(hb.SsmView(None, 0, 0, 0), n, ok2)}
        named = {"null weights": b"null pointer", "N = 65": b"SSM_ACC_WEIGHTS_MAX = 64", "a NaN weight": b"weight 1 must be finite",
                 "an infinite weight": b"weight 0 must be finite", "N = 0": b"bad sizes", "null src": b"null pointer"}
        for what, a in bad.items():
            rc = getattr(lib, entry)(*a, hb.stream_ptr())
            assert rc == -1, (entry, what)
            err = lib.ssm_last_error_string()
            assert entry[len("ssm_"):-len("_fwd")].encode() in err and named[what] in err, (entry, what, err)
        assert getattr(lib, entry)(*args(still, 64, fs(*([1.0] * 64))), hb.stream_ptr()) == 0, "64 weights are taken"
        torch.cuda.synchronize()
        acc.copy_(torch.from_numpy(before.view(np.float32))[:, :, 1:65, 4:68])
    torch.cuda.synchronize()
    for entry, args in entries.items():
        for wt in (None, fs(1.0, nan)):
            assert getattr(lib, entry)(*args(sv, n, wt), hb.stream_ptr()) == -1
    torch.cuda.synchronize()
    assert np.array_equal(bits(abuf.cpu().numpy()), before), "a refused call wrote the accumulator"
    assert np.array_equal(bits(src.cpu().numpy()), src_before), "a refused call wrote the frames"
    with pytest.raises(RuntimeError, match="SSM_ACC_WEIGHTS_MAX"):
        hb.frames_accumulate(src[:1].expand(65, -1, -1, -1), acc, 1, 1.0, weights=np.ones(65, np.float32))
    with pytest.raises(AssertionError, match="2 floats"):
        hb.frames_accumulate(src, acc, 1, 1.0, weights=np.ones(3, np.float32))


# ---- the streamed loop ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    return video_clips.synthetic_model(DEV)


def expected_stream(m, cfg, payloads, h, w, step, sigma, S, window, light=None):
    """tests/test_hip_shutter.py's composition with the window: ingest -> FullModel.interpolate of every running pair at its sample times,
    padded to `slots` -> the weighted yardstick over each output's samples in time order, one call per sample with its own weight, the
    window's scale on the last -> egress of the accumulator.  light: a curve's name, then in float64 through accumulate_light_host."""
    v = V()
    tl = v.Timeline(step, shutter=sigma, samples=S)
    n = len(payloads)
    dev = torch.from_numpy(payloads).to(DEV)
    matrix, crange = v.default_matrix(h), v.LIMITED
    planes = v.frames_from_yuv(dev, h, w, 0, matrix, crange, cfg, True)
    made = {}
    for i in range(n - 1):
        ts = [float(v.Timeline.t32(t)) for t, _, _ in tl.times(i)]
        if ts:
            x = v.frames_from_yuv(dev[i:i + 2], h, w, 0, matrix, crange, cfg, True)
            made[i] = m.interpolate(x[None], ts + [ts[-1]] * (tl.slots - len(ts))).cpu().numpy()
    planes = planes.cpu().numpy()
    wts, scale = v.shutter_window(window, S)
    out = []
    for smp in tl.outputs(n):
        acc = np.full((1,) + planes.shape[1:], np.nan, np.float32 if light is None else np.float64)
        for j, (i, t) in enumerate(smp):
            frame = planes[i] if t == 0 else made[i][[x for x, _, _ in tl.times(i)].index(t)]
            init, sc, last = 1 if j == 0 else 0, scale if j == S - 1 else 1.0, 1 if j == S - 1 else 0
            if light is None:
                v.accumulate_host(frame[None], acc, init, sc, weights=wts[j:j + 1])
            else:
                v.accumulate_light_host(frame[None], acc, init, sc, MEAN, STD, v.light_curve(light), last, weights=wts[j:j + 1])
        out.append(v.frames_to_yuv(torch.from_numpy(acc.astype(np.float32)).to(DEV), h, w, 0, matrix, crange, cfg).cpu().numpy()[0])
    return np.stack(out)


A = dict(target_rate=(24, 1), shutter=Fr(1, 2), shutter_samples=4)          # 60 -> 24: step 5/2; output 1 spans two pairs, passes and streams


@pytest.fixture(scope="module")
def payloads():
    return clip_payloads(N, H, W, 0)


@pytest.fixture(scope="module")
def box_run(model, payloads):
    cfg, m = model
    return stream(m, cfg, payloads, H, W, n_streams=2, pairs_per_batch=1, **A)


def test_triangle_stream_is_its_composition_and_differs_from_the_box(model, payloads, box_run):
    cfg, m = model
    hdr, got = stream(m, cfg, payloads, H, W, n_streams=2, pairs_per_batch=1, shutter_window="triangle", **A)
    assert got.shape[0] == 3 == V().Timeline(Fr(5, 2), shutter=Fr(1, 2), samples=4).n_outputs(N) and hdr.rate == (24, 1)
    want = expected_stream(m, cfg, payloads, H, W, Fr(5, 2), Fr(1, 2), 4, "triangle")
    assert np.array_equal(got, want), int((got != want).sum())
    assert got.shape == box_run[1].shape and not np.array_equal(got, box_run[1]), "weights (1, 3, 3, 1) / 8 are another picture than the box"


def test_samples_that_are_input_frames_get_their_weight(model, payloads):
    """Step 1/2 over the whole interval in 3 samples: every multiple of 1/6 is a sample, every input frame among them."""
    cfg, m = model
    hdr, got = stream(m, cfg, payloads, H, W, rate=(30, 1), n_streams=2, target_rate=(60, 1), shutter=1, shutter_samples=3, shutter_window="hann")
    assert hdr.rate == (60, 1) and got.shape[0] == 16
    want = expected_stream(m, cfg, payloads, H, W, Fr(1, 2), Fr(1), 3, "hann")
    assert np.array_equal(got, want), int((got != want).sum())


def test_windows_that_are_the_box(model, payloads, box_run):
    cfg, m = model
    two = dict(A, shutter_samples=2)
    _, box2 = stream(m, cfg, payloads, H, W, n_streams=2, **two)
    _, tri2 = stream(m, cfg, payloads, H, W, n_streams=2, shutter_window="triangle", **two)
    assert np.array_equal(tri2, box2), "triangle at S = 2 is (1, 1) with scale 1/2: the weighted kernels on the box's numbers"
    _, given = stream(m, cfg, payloads, H, W, n_streams=2, pairs_per_batch=1, shutter_window="box", **A)
    assert np.array_equal(given, box_run[1]), "box, given, is the default"


def test_one_sample_is_the_loop_without_a_shutter(model, payloads):
    cfg, m = model
    _, plain = stream(m, cfg, payloads, H, W, n_streams=2, target_rate=(24, 1))
    for window in ("hann", "gauss:3"):
        _, got = stream(m, cfg, payloads, H, W, n_streams=2, target_rate=(24, 1), shutter=Fr(1, 2), shutter_samples=1, shutter_window=window)
        assert np.array_equal(got, plain), window
        assert np.array_equal(got[0], payloads[0]) and np.array_equal(got[2], payloads[5]), "input frames pass through as their own bytes"


def test_window_in_light_is_its_composition_within_one_code(model, payloads):
    """The bar of tests/test_hip_shutter_light.py's stream test, for its reason: the kernel is within a bound of the float64 chain, not
    bit-equal to it, and a sample next to a rounding tie may come out as the neighbouring code."""
    cfg, m = model
    _, got = stream(m, cfg, payloads, H, W, n_streams=2, pairs_per_batch=1, shutter_light="srgb", shutter_window="triangle", **A)
    want = expected_stream(m, cfg, payloads, H, W, Fr(5, 2), Fr(1, 2), 4, "triangle", light="srgb")
    diff = np.abs(got.astype(int) - want.astype(int))
    print("srgb, triangle: %d of %d codes differ from the float64 chain, by %d at most" % (int((diff != 0).sum()), diff.size, int(diff.max())))
    assert got.shape == want.shape and diff.max() <= 1
    _, box = stream(m, cfg, payloads, H, W, n_streams=2, pairs_per_batch=1, shutter_light="srgb", **A)
    assert not np.array_equal(got, box)


def test_cli_round_trip(model, payloads, tmp_path, caplog):
    import logging
    import interpolate_video
    cfg, m = model
    v = V()
    src, dst, ini, logf = (str(tmp_path / x) for x in ("in.y4m", "out.y4m", "cfg.ini", "log.txt"))
    with open(src, "wb") as f:
        f.write(clip_file(payloads, H, W).getvalue())
    with open(ini, "w") as f:
        cfg.write(f)
    argv = ["-c", ini, "--expt", "t", "--log", logf, "--input", src, "--output", dst, "--fps", "24", "--shutter", "180", "--shutter_samples", "4",
            "--shutter_window", "gauss:2"]
    with caplog.at_level(logging.INFO):
        assert interpolate_video.main(argv, model=m) == 3
    hdr, got = read_clip(dst)
    assert got.shape[0] == 3 and hdr.rate == (24, 1) and (hdr.width, hdr.height) == (W, H), "the header's rate is what it is without --shutter"
    w, scale = v.shutter_window("gauss:2", 4)
    line = [x for x in caplog.messages if "shutter window:" in x]
    assert len(line) == 1 and "gauss:2" in line[0] and all("%.9g" % x in line[0] for x in w) and "scale %.9g" % scale in line[0], caplog.messages
    want = expected_stream(m, cfg, payloads, H, W, Fr(5, 2), Fr(1, 2), 4, "gauss:2")
    assert np.array_equal(got, want), int((got != want).sum())
