"""The shutter of the streamed video path on the GPU: ssm_frames_accumulate_fwd bit for bit against its numpy yardstick
(ssm_amd.video.accumulate_host), its refusals, and the streamed loop (VideoInterpolator(shutter=, shutter_samples=),
scripts/interpolate_video.py --shutter) byte for byte against the composition it stands for: ingest -> FullModel.interpolate of every
running pair at its sample times, padded to `slots` by repeating the last one -> accumulate_host over each output's samples in time
order -> egress of the accumulator.  The reference call uses `slots` times per call for the reason tests/test_hip_video_timeline.py gives:
a plan's tile choice depends on its batch.  The clip helpers are those of tests/video_clips.py, here on a 60:1 clip."""
import functools
import os
import sys
from fractions import Fraction as Fr

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import video_clips  # noqa: E402
from video_clips import V, clip_payloads, read_clip  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
H, W, N = 40, 48, 9          # canvas 64 x 64
clip_file = functools.partial(video_clips.clip_file, rate=(60, 1))
stream = functools.partial(video_clips.stream, rate=(60, 1))
POISON = np.uint32(0x7FC0DEAD)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- the kernel ----------------------------------------------------------------------------------------------------------------------
def mixed(rng, shape):
    """Both signs, magnitudes spread over 1e-3 .. 1e3."""
    return (rng.choice([-1.0, 1.0], shape) * 10.0 ** rng.uniform(-3, 3, shape)).astype(np.float32)


def poisoned(shape):
    return torch.from_numpy(np.full(shape, POISON, np.uint32).view(np.float32)).to(DEV)


def case(name, n, rng):
    """(src view [n,3,h,w], acc buffer, acc view [1,3,h,w] into it) on the device, the region filled with mixed values."""
    if name == "odd":            # 5 x 7 at an odd offset of a 16 x 24 canvas: nothing is aligned, one element per lane
        sbuf, abuf = poisoned((n, 3, 16, 24)), poisoned((1, 3, 16, 24))
        src, acc = sbuf[:, :, 3:8, 5:12], abuf[:, :, 3:8, 5:12]
    elif name == "aligned":      # 64 x 64 at (1, 4) of a 66 x 72 buffer: 16-byte aligned rows, strides of multiples of 4
        sbuf, abuf = poisoned((n, 3, 66, 72)), poisoned((1, 3, 66, 72))
        src, acc = sbuf[:, :, 1:65, 4:68], abuf[:, :, 1:65, 4:68]
        assert src.data_ptr() % 16 == 0 and acc.data_ptr() % 16 == 0
    else:                        # frames of a [n,2,3,64,64] tensor: the batch stride is twice C H W
        sbuf, abuf = poisoned((n, 2, 3, 64, 64)), poisoned((1, 3, 66, 72))
        src, acc = sbuf[:, 1], abuf[:, :, 1:65, 4:68]
        assert src.stride(0) == 2 * 3 * 64 * 64
    src.copy_(torch.from_numpy(mixed(rng, tuple(src.shape))))
    acc.copy_(torch.from_numpy(mixed(rng, tuple(acc.shape))))
    return src, abuf, acc


@pytest.mark.parametrize("name", ["odd", "aligned", "strided"])
def test_accumulate_is_bit_equal_to_the_yardstick(name):
    from ssm_amd import hipbind as hb
    v = V()
    rng = np.random.default_rng(11)
    for n in (1, 2, 7):
        for init in (0, 1):
            for scale in (1.0, np.float32(1.0 / 3.0), 0.125):
                src, abuf, acc = case(name, n, rng)
                want_buf = abuf.cpu().numpy()
                region = tuple(slice(o, o + s) for o, s in zip((0, 0) + ((3, 5) if name == "odd" else (1, 4)), acc.shape))
                want = v.accumulate_host(src.cpu().numpy(), np.ascontiguousarray(want_buf[region]), init, scale)
                want_buf[region] = want
                assert hb.frames_accumulate(src, acc, init, scale) is acc
                torch.cuda.synchronize()
                got_buf = abuf.cpu().numpy()
                assert np.array_equal(bits(got_buf[region]), bits(want)), (n, init, scale, int((bits(got_buf[region]) != bits(want)).sum()))
                assert np.array_equal(bits(got_buf), bits(want_buf)), "an element outside the region lost its poison bits"
                assert int((bits(got_buf) == POISON).sum()) == got_buf.size - acc.numel()


def test_accumulate_refusals_leave_the_accumulator_alone():
    import ctypes
    from ssm_amd import hipbind as hb
    lib = hb.load()
    rng = np.random.default_rng(3)
    src, abuf, acc = case("aligned", 2, rng)
    before = bits(abuf.cpu().numpy()).copy()
    sv, av, null = hb.view_of(src), hb.view_of(acc), hb.SsmView(None, 0, 0, 0)
    n, c, h, w = src.shape
    still = hb.SsmView(src.data_ptr(), 0, src.stride(1), src.stride(2))          # every frame the first one: no size reaches past the buffer
    short_s = hb.SsmView(src.data_ptr(), src.stride(0), src.stride(1), w - 1)
    short_a = hb.SsmView(acc.data_ptr(), acc.stride(0), acc.stride(1), w - 1)
    inside = hb.view_of(src[1:2])                                                 # an accumulator that is one of the frames
    astride = hb.view_of(src[0:1, :, 32:, :])                                     # ... or the lower half of one, as [1,3,32,64]
    f = ctypes.c_float
    bad = {"null src": (null, av, n, c, h, w, 1, f(1.0)), "null acc": (sv, null, n, c, h, w, 1, f(1.0)),
           "N = 0": (sv, av, 0, c, h, w, 1, f(1.0)), "C = 0": (sv, av, n, 0, h, w, 1, f(1.0)), "H = 0": (sv, av, n, c, 0, w, 1, f(1.0)),
           "W = 0": (sv, av, n, c, h, 0, 1, f(1.0)), "N = -1": (sv, av, -1, c, h, w, 1, f(1.0)),
           "N = 65536": (still, av, 65536, c, h, w, 1, f(1.0)),
           "short src rows": (short_s, av, n, c, h, w, 1, f(1.0)), "short acc rows": (sv, short_a, n, c, h, w, 1, f(1.0)),
           "init = 2": (sv, av, n, c, h, w, 2, f(1.0)), "init = -1": (sv, av, n, c, h, w, -1, f(1.0)),
           "scale nan": (sv, av, n, c, h, w, 1, f(float("nan"))), "scale inf": (sv, av, n, c, h, w, 0, f(float("inf"))),
           "acc among the frames": (sv, inside, n, c, h, w, 1, f(1.0)), "acc inside a frame": (sv, astride, n, c, 32, w, 0, f(1.0))}
    src_before = bits(src.cpu().numpy()).copy()
    for what, args in bad.items():
        rc = lib.ssm_frames_accumulate_fwd(*args, hb.stream_ptr())
        assert rc == -1, what
        assert b"frames_accumulate" in lib.ssm_last_error_string(), what
    torch.cuda.synchronize()
    assert np.array_equal(bits(abuf.cpu().numpy()), before), "a refused call wrote the accumulator"
    assert np.array_equal(bits(src.cpu().numpy()), src_before), "a refused call wrote the frames"
    with pytest.raises(RuntimeError, match="overlap"):
        hb.frames_accumulate(src, src[1:2], 1, 1.0)


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


def expected_stream(m, cfg, payloads, h, w, step, sigma, S, **mode):
    v = V()
    tl = v.Timeline(step, shutter=sigma, samples=S)
    n = len(payloads)
    dev = torch.from_numpy(payloads).to(DEV)
    matrix, crange, mult = v.default_matrix(h), v.LIMITED, 32 * mode.get("flow_scale", 1)
    planes = v.frames_from_yuv(dev, h, w, 0, matrix, crange, cfg, True, multiple=mult)
    made = {}
    for i in range(n - 1):
        ts = [float(v.Timeline.t32(t)) for t, _, _ in tl.times(i)]
        if ts:
            x = v.frames_from_yuv(dev[i:i + 2], h, w, 0, matrix, crange, cfg, True, multiple=mult)
            made[i] = m.interpolate(x[None], ts + [ts[-1]] * (tl.slots - len(ts)), **mode).cpu().numpy()
    planes = planes.cpu().numpy()
    scale = np.float32(1.0 / S)
    out = []
    for smp in tl.outputs(n):
        acc = np.full((1,) + planes.shape[1:], np.nan, np.float32)
        for j, (i, t) in enumerate(smp):
            frame = planes[i] if t == 0 else made[i][[x for x, _, _ in tl.times(i)].index(t)]
            v.accumulate_host(frame[None], acc, 1 if j == 0 else 0, scale if j == S - 1 else 1.0)
        out.append(v.frames_to_yuv(torch.from_numpy(acc).to(DEV), h, w, 0, matrix, crange, cfg).cpu().numpy()[0])
    return np.stack(out)


A = dict(target_rate=(24, 1), shutter=Fr(1, 2), shutter_samples=4)          # 60 -> 24: step 5/2


@pytest.fixture(scope="module")
def case_a(model):
    """The 9-frame clip and its 60 -> 24 output at 180 degrees in 4 samples, 2 streams, one pair per pass: computed once, read by three tests."""
    cfg, m = model
    payloads = clip_payloads(N, H, W, 0)
    return payloads, stream(m, cfg, payloads, H, W, n_streams=2, pairs_per_batch=1, **A)


def test_outputs_that_span_pairs_passes_and_streams(model, case_a):
    """(a) taus 0 5/16 10/16 15/16 | 2.5 2.8125 3.125 3.4375 | 5 ... : output 0 is frame 0 and three frames of pair 0, output 1 two frames
    of pair 2 and two of pair 3 - two passes, on two streams."""
    cfg, m = model
    payloads, (hdr, got) = case_a
    assert got.shape[0] == 3 == V().Timeline(Fr(5, 2), shutter=Fr(1, 2), samples=4).n_outputs(N) and hdr.rate == (24, 1)
    want = expected_stream(m, cfg, payloads, H, W, Fr(5, 2), Fr(1, 2), 4)
    assert np.array_equal(got, want), int((got != want).sum())
    assert not np.array_equal(got[0], payloads[0]), "output 0 is a mean, not frame 0"
    _, sharp = stream(m, cfg, payloads, H, W, n_streams=2, target_rate=(24, 1))
    assert np.array_equal(sharp[0], payloads[0]) and not np.array_equal(sharp[1], got[1])


def test_samples_that_are_input_frames(model):
    """(b) step 1/2 over the whole interval in 3 samples: every multiple of 1/6 is a sample, every input frame among them."""
    cfg, m = model
    payloads = clip_payloads(N, H, W, 0)
    hdr, got = stream(m, cfg, payloads, H, W, rate=(30, 1), n_streams=2, target_rate=(60, 1), shutter=1, shutter_samples=3)
    assert hdr.rate == (60, 1) and got.shape[0] == 16 == V().Timeline(Fr(1, 2), shutter=1, samples=3).n_outputs(N)
    want = expected_stream(m, cfg, payloads, H, W, Fr(1, 2), Fr(1), 3)
    assert np.array_equal(got, want), int((got != want).sum())


def test_coarse_flow_mode(model):
    """(c) case (a) with flow_scale = 2 on a 96 x 80 clip (canvas 128 x 128)."""
    cfg, m = model
    h, w = 80, 96
    payloads = clip_payloads(N, h, w, 0)
    hdr, got = stream(m, cfg, payloads, h, w, n_streams=2, flow_scale=2, **A)
    want = expected_stream(m, cfg, payloads, h, w, Fr(5, 2), Fr(1, 2), 4, flow_scale=2)
    assert got.shape[0] == 3 and np.array_equal(got, want), int((got != want).sum())


def test_two_pairs_per_pass(model, case_a):
    cfg, m = model
    payloads, (_, ref) = case_a
    hdr, got = stream(m, cfg, payloads, H, W, n_streams=2, pairs_per_batch=2, **A)
    assert got.shape == ref.shape
    # the bound of tests/test_hip_video.py test_batched_passes_keep_count_order_and_originals, for its reason: a two-pair pass runs its
    # convolutions at twice the batch, where the plan may pick other tiles; fp32 sums in another order can flip a code only at a tie
    diff = np.abs(got.astype(int) - ref.astype(int))
    print("two pairs per pass: %d codes differ, by %d at most" % (int((diff != 0).sum()), int(diff.max())))
    assert diff.max() <= 1


def test_one_sample_is_the_loop_without_a_shutter(model):
    cfg, m = model
    payloads = clip_payloads(N, H, W, 0)
    _, plain = stream(m, cfg, payloads, H, W, n_streams=2, target_rate=(24, 1))
    hdr, got = stream(m, cfg, payloads, H, W, n_streams=2, target_rate=(24, 1), shutter=Fr(1, 2), shutter_samples=1)
    assert hdr.rate == (24, 1) and np.array_equal(got, plain)
    assert np.array_equal(got[0], payloads[0]) and np.array_equal(got[2], payloads[5]), "input frames pass through as their own bytes"


def test_device_memory_is_flat_in_clip_length(model):
    cfg, m = model
    v = V()
    vi = v.VideoInterpolator(m, cfg, n_streams=2, pairs_per_batch=1, **A)
    tl = v.Timeline(Fr(5, 2), shutter=Fr(1, 2), samples=4)
    peaks = []
    for n in (9, 9, 40):          # the first run also builds the plans
        r = v.Y4MReader(clip_file(clip_payloads(n, H, W, 0), H, W))
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(DEV)
        sink = open(os.devnull, "wb")
        assert vi.run(r, v.Y4MWriter.like(sink, r, rate=(24, 1))) == tl.n_outputs(n)
        sink.close()
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated(DEV))
    print("peak device memory: 9 frames %d B, 40 frames %d B" % (peaks[1], peaks[2]))
    assert peaks[2] == peaks[1], peaks


def test_cli_round_trip(model, tmp_path):
    import interpolate_video
    cfg, m = model
    v = V()
    payloads = clip_payloads(N, H, W, 0)
    src, dst, ini, logf = (str(tmp_path / x) for x in ("in.y4m", "out.y4m", "cfg.ini", "log.txt"))
    with open(src, "wb") as f:
        f.write(clip_file(payloads, H, W).getvalue())
    with open(ini, "w") as f:
        cfg.write(f)
    argv = ["-c", ini, "--expt", "t", "--log", logf, "--input", src, "--output", dst, "--fps", "24", "--shutter", "180", "--shutter_samples", "4"]
    count = v.Timeline(Fr(5, 2), shutter=Fr(1, 2), samples=4).n_outputs(N)
    assert interpolate_video.main(argv, model=m) == count == 3
    hdr, got = read_clip(dst)
    assert got.shape[0] == count and hdr.rate == (24, 1) and (hdr.width, hdr.height) == (W, H)
    assert not np.array_equal(got[0], payloads[0]), "with a shutter even output 0 comes from the accumulator"
