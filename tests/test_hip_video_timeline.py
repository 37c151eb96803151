"""The streamed loop on an arbitrary timeline (VideoInterpolator(target_rate=, speed=), scripts/interpolate_video.py --fps / --speed)
against the expected stream: for every pair that gets a frame, ingest -> FullModel.interpolate at the pair's times, padded to `slots` by
repeating the last one -> egress of the frames the timeline asks for; frames at integer times are their input bytes.  The reference call
uses `slots` times per call because a plan's tile choice depends on its batch: at the same number of times per call the streamed loop
and the call run the same kernels on the same numbers, hence BYTE equality.  The clip helpers are those of tests/video_clips.py."""
import os
import sys
from fractions import Fraction as Fr

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from video_clips import V, clip_file, clip_payloads, read_clip, stream  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
H, W, N = 64, 96, 6


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


def expected_stream(m, cfg, payloads, h, w, siting, step, **mode):
    v = V()
    tl = v.Timeline(step)
    dev = torch.from_numpy(payloads).to(DEV)
    matrix, crange = v.default_matrix(h), v.LIMITED
    out, made = [], {}
    for i, t in tl.outputs(len(payloads)):
        if t == 0:
            out.append(payloads[i])
            continue
        if i not in made:
            ts = [float(v.Timeline.t32(x)) for x in tl.times(i)]
            x = v.frames_from_yuv(dev[i:i + 2], h, w, siting, matrix, crange, cfg, True, multiple=32 * mode.get("flow_scale", 1))
            frames = m.interpolate(x[None], ts + [ts[-1]] * (tl.slots - len(ts)), **mode)
            made[i] = list(v.frames_to_yuv(frames[:len(ts)], h, w, siting, matrix, crange, cfg).cpu().numpy())
        out.append(made[i].pop(0))
    assert not any(made.values())
    return np.stack(out)


@pytest.fixture(scope="module")
def clip_30_to_75(model):
    """The 6-frame 4:2:0 clip and its 30 -> 75 output at one pair per pass: computed once, read by three tests."""
    cfg, m = model
    payloads = clip_payloads(N, H, W, 0)
    return payloads, stream(m, cfg, payloads, H, W, n_streams=2, target_rate=(75, 1))


def test_30_to_75(model, clip_30_to_75):
    cfg, m = model
    payloads, (hdr, got) = clip_30_to_75
    assert got.shape[0] == 13 and hdr.rate == (75, 1) and hdr.chroma == "420jpeg"
    assert np.array_equal(got[::5], payloads[::2]), "frames at integer tau are the input frames' own bytes"
    want = expected_stream(m, cfg, payloads, H, W, 0, Fr(2, 5))
    assert np.array_equal(got, want), int((got != want).sum())
    assert not np.array_equal(got[1], got[2]) and not np.array_equal(got[1], payloads[0])


def test_step_one_quarter_is_upsample_rate_4(model):
    cfg, m = model
    payloads = clip_payloads(N, H, W, 0)
    hdr, got = stream(m, cfg, payloads, H, W, target_rate=(120, 1))
    hdr4, got4 = stream(m, cfg, payloads, H, W, upsample_rate=4)
    assert hdr.rate == (120, 1) and got.shape[0] == (N - 1) * 4 + 1
    assert np.array_equal(got, got4), int((got != got4).sum())


def test_step_above_one_skips_pairs_and_frames(model):
    """step = 6/5 over 8 frames: taus 0 6/5 12/5 18/5 24/5 6 - pairs 0, 5 and 6 get nothing and are not run (frames 0 and 6 are written
    from the host buffer without going up), and frame 7 is needed by no output: other bytes in it change nothing."""
    cfg, m = model
    v = V()
    n = 8
    payloads = clip_payloads(n, H, W, v.C444)
    hdr, got = stream(m, cfg, payloads, H, W, "444", n_streams=1, speed=Fr(6, 5))
    assert hdr.rate == (30, 1) and hdr.chroma == "444" and got.shape[0] == 6 == v.Timeline(Fr(6, 5)).n_outputs(n)
    assert np.array_equal(got[0], payloads[0]) and np.array_equal(got[5], payloads[6])
    want = expected_stream(m, cfg, payloads, H, W, v.C444, Fr(6, 5))
    assert np.array_equal(got, want), int((got != want).sum())
    poisoned = payloads.copy()
    poisoned[7] = 255 - poisoned[7]
    _, again = stream(m, cfg, poisoned, H, W, "444", n_streams=1, speed=Fr(6, 5))
    assert np.array_equal(again, got), "a frame that no output needs must not change anything"


def test_50_to_60(model):
    cfg, m = model
    v = V()
    payloads = clip_payloads(N, H, W, v.COSITED)
    hdr, got = stream(m, cfg, payloads, H, W, "420mpeg2", rate=(50, 1), n_streams=3, target_rate=(60, 1))
    assert hdr.rate == (60, 1) and got.shape[0] == 7
    assert np.array_equal(got[0], payloads[0]) and np.array_equal(got[6], payloads[5])
    want = expected_stream(m, cfg, payloads, H, W, v.COSITED, Fr(5, 6))
    assert np.array_equal(got, want), int((got != want).sum())


def test_speed_alone_keeps_the_rate(model):
    cfg, m = model
    payloads = clip_payloads(N, H, W, 0)
    hdr, got = stream(m, cfg, payloads, H, W, speed="3/10")
    assert hdr.rate == (30, 1) and got.shape[0] == 17          # floor(5 / 0.3) + 1
    assert np.array_equal(got[10], payloads[3])                # tau = 3
    want = expected_stream(m, cfg, payloads, H, W, 0, Fr(3, 10))
    assert np.array_equal(got, want), int((got != want).sum())


def test_two_pairs_per_pass(model, clip_30_to_75):
    cfg, m = model
    payloads, (_, ref) = clip_30_to_75
    hdr, got = stream(m, cfg, payloads, H, W, n_streams=2, pairs_per_batch=2, target_rate=(75, 1))
    assert got.shape[0] == 13 and np.array_equal(got[::5], payloads[::2])
    # the bound of tests/test_hip_video.py test_batched_passes_keep_count_order_and_originals, for its reason: a two-pair pass runs its
    # convolutions at batch 4 instead of 2, where the plan may pick other tiles; fp32 sums in another order can flip a code only at a tie
    diff = np.abs(got.astype(int) - ref.astype(int))
    print("two pairs per pass: %d codes differ, by %d at most" % (int((diff != 0).sum()), int(diff.max())))
    assert diff.max() <= 1


def test_coarse_flow_mode(model):
    """flow_scale = 2 at 64 x 64, the smallest canvas of that mode (multiples of 32 * flow_scale)."""
    cfg, m = model
    h = w = 64
    payloads = clip_payloads(N, h, w, 0)
    hdr, got = stream(m, cfg, payloads, h, w, flow_scale=2, target_rate=(75, 1))
    want = expected_stream(m, cfg, payloads, h, w, 0, Fr(2, 5), flow_scale=2)
    assert got.shape[0] == 13 and np.array_equal(got, want), int((got != want).sum())


def test_tiled_mode(model):
    """64 x 192 in tiles of 64 x 96: the smallest tiling that makes two windows."""
    cfg, m = model
    h, w, tiling = 64, 192, dict(tile=(64, 96), halo=32, blend=8)
    payloads = clip_payloads(N, h, w, 0)
    hdr, got = stream(m, cfg, payloads, h, w, target_rate=(75, 1), **tiling)
    want = expected_stream(m, cfg, payloads, h, w, 0, Fr(2, 5), **tiling)
    assert got.shape[0] == 13 and np.array_equal(got, want), int((got != want).sum())


def test_device_memory_is_flat_in_clip_length(model):
    cfg, m = model
    v = V()
    vi = v.VideoInterpolator(m, cfg, n_streams=2, pairs_per_batch=1, target_rate=(75, 1))
    peaks = []
    for n in (8, 8, 40):          # the first run also builds the plans
        r = v.Y4MReader(clip_file(clip_payloads(n, H, W, 0), H, W))
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(DEV)
        sink = open(os.devnull, "wb")
        assert vi.run(r, v.Y4MWriter.like(sink, r, rate=(75, 1))) == (n - 1) * 5 // 2 + 1
        sink.close()
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated(DEV))
    print("peak device memory: 8 frames %d B, 40 frames %d B" % (peaks[1], peaks[2]))
    assert peaks[2] <= peaks[1], peaks


@pytest.mark.parametrize("flags,count,rate", [(["--fps", "75"], 6, (75, 1)), (["--speed", "1/4"], 9, (30, 1))])
def test_cli_end_to_end(model, tmp_path, flags, count, rate):
    import interpolate_video
    cfg, m = model
    h, w, n = 40, 56, 3
    payloads = clip_payloads(n, h, w, 0)
    src, dst, ini, logf = (str(tmp_path / x) for x in ("in.y4m", "out.y4m", "cfg.ini", "log.txt"))
    with open(src, "wb") as f:
        f.write(clip_file(payloads, h, w).getvalue())
    with open(ini, "w") as f:
        cfg.write(f)
    argv = ["-c", ini, "--expt", "t", "--log", logf, "--input", src, "--output", dst] + flags
    assert interpolate_video.main(argv, model=m) == count
    hdr, got = read_clip(dst)
    assert got.shape[0] == count and hdr.rate == rate and (hdr.width, hdr.height) == (w, h)
    assert np.array_equal(got[0], payloads[0]) and np.array_equal(got[-1], payloads[2])
    assert not any(np.array_equal(got[1], p) for p in payloads), "the second frame is a synthesised one"
