"""The evaluator's PSNR / SSIM / IE on the GPU (csrc/ssm_metrics.hip through ssm_amd.evaluation.frame_metrics) against the host
functions psnr / ssim / interpolation_error, which stay the yardstick: PSNR bit for bit, IE to 1e-12 relative, SSIM to 1e-9
absolute.  Then repeatability (bitwise, independent of the batch and the stream), argument checks and the Evaluator's
metrics="device" switch."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def host_metrics(t, o):
    from ssm_amd.evaluation import interpolation_error, psnr, ssim
    return psnr(t, o), ssim(t, o), interpolation_error(t, o)


def check_against_host(t, o):
    """t, o: host uint8 [N,H,W,3]; frame_metrics on the device copies against the host metrics frame by frame."""
    from ssm_amd.evaluation import frame_metrics
    got = frame_metrics(torch.from_numpy(t).to(DEV), torch.from_numpy(o).to(DEV))
    assert got.shape == (t.shape[0], 3) and got.dtype == np.float64
    for k in range(t.shape[0]):
        p, s, e = host_metrics(t[k], o[k])
        assert got[k, 0] == p or (np.isinf(p) and np.isinf(got[k, 0])), (t.shape, k, got[k, 0], p)
        assert abs(got[k, 1] - s) <= 1e-9, (t.shape, k, got[k, 1], s)
        assert abs(got[k, 2] - e) <= 1e-12 * abs(e), (t.shape, k, got[k, 2], e)
    return got


def random_pair(n, h, w, seed):
    rng = np.random.RandomState(seed)
    return rng.randint(0, 256, (n, h, w, 3)).astype(np.uint8), rng.randint(0, 256, (n, h, w, 3)).astype(np.uint8)


@pytest.mark.parametrize("h,w", [(11, 11), (12, 37), (60, 90), (33, 130), (256, 448)])
@pytest.mark.parametrize("n", [1, 9])
def test_random_frames_match_host(h, w, n):
    """Ragged tiles in both directions, a frame narrower than one tile, the minimum size the 11x11 window allows."""
    t, o = random_pair(n, h, w, seed=h * 1000 + w + n)
    check_against_host(t, o)


def test_synthetic_clip_pairs_match_host():
    from ssm_amd.weights import synthetic_frames_u8
    clip = synthetic_frames_u8(6, 72, 104, seed=5).permute(0, 2, 3, 1).contiguous().numpy()
    check_against_host(clip[:-1].copy(), clip[1:].copy())


def test_flat_frames_stress_the_variance_cancellation():
    rng = np.random.RandomState(2)
    flat = np.full((3, 47, 70, 3), 200, np.uint8)
    flat[1] = 3
    flat[2] = 128
    noisy = np.clip(flat.astype(int) + rng.randint(-2, 3, flat.shape), 0, 255).astype(np.uint8)
    check_against_host(flat, flat + 1)
    check_against_host(flat, noisy)


def test_checkerboards_stress_saturation_and_the_frame_edges():
    """0/255 patterns: the largest differences and variances, a 29x45 frame whose tiles are ragged in both directions.  The summed
    SSIM interior reads no reflected pixel, so this checks the border mask and the clamped edge reads, not the reflection itself."""
    cb = ((np.indices((29, 45)).sum(0) % 2) * 255).astype(np.uint8)[..., None].repeat(3, 2)
    stripes = ((np.arange(45)[None, :, None] // 3 % 2) * 255).repeat(29, 0).repeat(3, 2).astype(np.uint8)
    t = np.stack([cb, cb, stripes, cb])
    o = np.stack([255 - cb, np.roll(cb, 1, axis=0), 255 - stripes, np.zeros_like(cb)])
    check_against_host(t, o)


def test_identical_frames():
    from ssm_amd.evaluation import frame_metrics
    t, _ = random_pair(3, 40, 77, seed=4)
    got = frame_metrics(torch.from_numpy(t).to(DEV), torch.from_numpy(t).to(DEV))
    assert np.isinf(got[:, 0]).all() and (got[:, 2] == 0.0).all()
    assert np.abs(got[:, 1] - 1.0).max() <= 1e-12, got[:, 1]


def test_sums_are_repeatable_and_independent_of_the_batch_and_stream():
    from ssm_amd.evaluation import frame_metric_sums
    t, o = random_pair(9, 83, 150, seed=6)
    td, od = torch.from_numpy(t).to(DEV), torch.from_numpy(o).to(DEV)
    a = frame_metric_sums(td, od).cpu()
    b = frame_metric_sums(td, od).cpu()
    assert torch.equal(a, b)
    for k in (0, 4, 8):
        alone = frame_metric_sums(td[k:k + 1], od[k:k + 1]).cpu()
        assert torch.equal(alone[0], a[k]), k
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        c = frame_metric_sums(td, od)
    torch.cuda.current_stream().wait_stream(s)
    assert torch.equal(c.cpu(), a)
    assert (a[:, 0] == torch.round(a[:, 0])).all(), "the SSE is an exact integer"


def test_argument_checks():
    from ssm_amd.evaluation import frame_metric_sums
    small = torch.zeros(1, 10, 40, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="smaller than the 11x11"):
        frame_metric_sums(small, small)
    narrow = torch.zeros(1, 40, 10, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="smaller than the 11x11"):
        frame_metric_sums(narrow, narrow)
    a = torch.zeros(2, 32, 32, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="differ"):
        frame_metric_sums(a, a[:1])
    with pytest.raises(RuntimeError, match="uint8"):
        frame_metric_sums(a, a.float())
    with pytest.raises(RuntimeError, match="on the GPU"):
        frame_metric_sums(a.cpu(), a.cpu())
    with pytest.raises(RuntimeError, match="on the GPU"):
        frame_metric_sums(a[..., :2], a[..., :2])


def test_evaluator_device_metrics_match_host_metrics():
    """The 12-image 60x90 clip of test_frames_eval.test_evaluator_loop_on_a_synthetic_clip through both Evaluator modes."""
    from models.superslomo_r import FullModel
    from ssm_amd.config import load_config, synthetic_weight_overrides
    from ssm_amd.evaluation import Evaluator, clip_samples
    from ssm_amd.weights import synthetic_frames_u8, synthetic_state_dict
    cfg = load_config("superslomo_original.ini", synthetic_weight_overrides())
    m = FullModel(cfg)
    m.stage1_model.load_state_dict(synthetic_state_dict(1))
    m.stage2_model.load_state_dict(synthetic_state_dict(2))
    m = m.to(DEV).eval()
    h, w = 60, 90
    clip = synthetic_frames_u8(12, h, w, seed=11).permute(0, 2, 3, 1).contiguous().to(DEV)
    res = {}
    evs = {}
    for mode in ("host", "device"):
        evs[mode] = Evaluator(cfg, m, h, w, dataset="ADOBE", metrics=mode)
        res[mode] = evs[mode].run_evaluation(clip_samples(clip, cfg, n_frames=2))
    hv, dv = evs["host"], evs["device"]
    assert res["host"]["frames"] == res["device"]["frames"] == 10
    assert dv.video_PSNR == hv.video_PSNR
    assert all(type(v) is float for v in dv.video_PSNR + dv.video_IE + dv.video_SSIM)
    np.testing.assert_allclose(dv.video_IE, hv.video_IE, rtol=1e-12, atol=0)
    np.testing.assert_allclose(dv.video_SSIM, hv.video_SSIM, rtol=0, atol=1e-9)


def test_sintel_sized_frames_match_host():
    """436x1024, the SINTEL_HFR frame size: a textured pair and a slightly perturbed copy."""
    from ssm_amd.weights import synthetic_frames_u8
    clip = synthetic_frames_u8(2, 436, 1024, seed=9).permute(0, 2, 3, 1).contiguous().numpy()
    rng = np.random.RandomState(1)
    near = np.clip(clip[:1].astype(int) + rng.randint(-4, 5, clip[:1].shape), 0, 255).astype(np.uint8)
    check_against_host(np.concatenate([clip[:1], clip[:1]]), np.concatenate([clip[1:], near]))


def test_frame_metrics_against_host_720p():
    """7 frames at 720x1280, the batch size of one ADOBE window."""
    from ssm_amd.weights import synthetic_frames_u8
    clip = synthetic_frames_u8(8, 720, 1280, seed=3).permute(0, 2, 3, 1).contiguous().numpy()
    check_against_host(clip[:-1].copy(), clip[1:].copy())
