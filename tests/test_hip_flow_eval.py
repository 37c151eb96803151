"""Optical-flow evaluation on the GPU (csrc/ssm_flow.hip through ssm_amd.flow_eval, FullModel.estimate_flow) against its host
yardsticks: the reference's recorded outputs in tests/golden/flow_eval.npz, compute_metrics_host and scripts/utils/flo_utils.py.

Bars.  Both counts of the metric record (pixels > 3 px off, pixels counted) are exact integers and must be EQUAL: the kernel forms
the per-pixel error with the same un-fused float32 operations numpy uses, and the tests assert that no error of their fields lies
within 1e-4 of 3.0 in a float64 evaluation, so the count does not hang on a last bit.  The EPE sum is held to 1e-12 relative of a
float64 sum of the yardstick's float32 error map (an fp64 tree sum of < 2^20 terms is orders inside it), the EPE mean to 2e-6
relative of the reference's float32 np.mean (pairwise float32 summation over 4.5e5 terms carries about log2(n) * 2^-24 = 1.2e-6:
the yardstick's rounding).  Colour maps: every channel of every pixel within 1 level of the reference's image, black exactly where
the flow is unknown or NaN; the rad <= 1 branch is bit-exact by construction, so only the last bits of a float64 angle differ.
estimate_flow is the same kernels on the same inputs as the full forward's stage 1: bitwise equal."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
N_METRIC, N_COLOUR = 4, 6


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def planar(flow_hw2):
    """host [N,H,W,2] -> device [N,2,H,W]"""
    return T(np.moveaxis(np.asarray(flow_hw2), 3, 1))


def make_model(precision=None):
    from models.superslomo_r import FullModel
    from ssm_amd.config import load_config, synthetic_weight_overrides
    from ssm_amd.weights import synthetic_state_dict
    cfg = load_config("superslomo_original.ini", synthetic_weight_overrides())
    m = FullModel(cfg)
    m.stage1_model.load_state_dict(synthetic_state_dict(1))
    m.stage2_model.load_state_dict(synthetic_state_dict(2))
    m.precision = precision
    return cfg, m.to(DEV).eval()


def host_record(flow, gt, mode):
    """(float32 error map, counted mask, float64 sum, count > 3, count) of one [H,W,2] pair - the yardstick of ssm_flow_metrics_fwd."""
    from ssm_amd.flow_eval import error_map_host
    err = error_map_host(flow, gt)
    if mode == 0:
        counted = np.ones(err.shape, bool)
    else:
        unknown = (np.abs(gt[..., 0]) > 1e7) | (np.abs(gt[..., 1]) > 1e7)
        counted = ~unknown & ((np.abs(gt[..., 0]) > 0) | (np.abs(gt[..., 1]) > 0))
    return err, counted, float(err[counted].astype(np.float64).sum()), int((err[counted] > 3).sum()), int(counted.sum())


def assert_clear_of_three(flow, gt):
    d = gt.astype(np.float64) - flow.astype(np.float64)
    err = np.sqrt((d * d).sum(axis=2))
    gap = np.abs(err[np.isfinite(err)] - 3.0).min()
    assert gap >= 1e-4, "a pixel error lies %.3g from 3.0: the exact count would hang on rounding" % gap


def check_metric_sums(sums, flows, gts, mode, recorded=None):
    """sums: host [N,3] float64 from the device; flows / gts: host [N,H,W,2]."""
    assert sums.shape == (len(flows), 3) and sums.dtype == np.float64
    for k in range(len(flows)):
        assert_clear_of_three(flows[k], gts[k])
        err, counted, want_sum, want_over, want_n = host_record(flows[k], gts[k], mode)
        rel = abs(sums[k, 0] - want_sum) / abs(want_sum)
        print("mode %d field %d %s: sum %.17g (host %.17g, rel %.2e), > 3: %d (host %d), counted %d (host %d)"
              % (mode, k, err.shape, sums[k, 0], want_sum, rel, sums[k, 1], want_over, sums[k, 2], want_n))
        assert sums[k, 1] == want_over and sums[k, 2] == want_n, (mode, k, sums[k], want_over, want_n)
        assert rel <= 1e-12, (mode, k, sums[k, 0], want_sum)
        mean32 = np.mean(err[counted])                                     # the reference's float32 np.mean
        assert abs(sums[k, 0] / sums[k, 2] - float(mean32)) <= 2e-6 * float(mean32), (mode, k, sums[k, 0] / sums[k, 2], mean32)
        if recorded is not None:
            want = float(recorded[k])
            assert abs(sums[k, 0] / sums[k, 2] - want) <= 2e-6 * want, (mode, k, sums[k, 0] / sums[k, 2], want)


@pytest.mark.parametrize("mode", [0, 1])
def test_metric_kernel_matches_the_reference_on_the_fixture_fields(golden, mode):
    from ssm_amd.flow_eval import flow_metric_sums, flow_metrics
    g = golden("flow_eval")
    key = "m%d_epe" if mode == 0 else "m%d_epe_mode1"
    for ks in ((0, 2, 3), (1,)):                                           # the three 54 x 128 fields as one batch, the ragged one alone
        flows = np.stack([g["m%d_flow" % k] for k in ks])
        gts = np.stack([g["m%d_gt" % k] for k in ks])
        sums = flow_metric_sums(planar(flows), T(gts), 0, 0, mode).cpu().numpy()
        check_metric_sums(sums, flows, gts, mode, recorded=[g[key % k] for k in ks])
        if mode == 0:
            m = flow_metrics(planar(flows), T(gts))
            for j, k in enumerate(ks):
                assert m[j, 1] == float(g["m%d_pct" % k]), (k, m[j, 1], g["m%d_pct" % k])     # the reference's own division: exact


def sintel_sized_case(seed):
    """A 436 x 1024 flow pair whose errors keep clear of 3.0: the error vector is drawn first (radius in [0, 8) with (2.99, 3.01)
    cut out), the flow is ground truth minus it.  The ground truth has a zero rectangle and unknown pixels for mode 1."""
    rng = np.random.RandomState(seed)
    h, w = 436, 1024
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    gt = np.stack([12 * np.sin(0.011 * x + 0.02 * y + seed) + 3 * np.cos(0.05 * y), 9 * np.cos(0.013 * x - 0.017 * y) + 0.01 * x],
                  axis=2).astype(np.float32)
    r = rng.uniform(0, 8, (h, w))
    r = np.where(np.abs(r - 3.0) < 0.01, r + 0.02, r)
    th = rng.uniform(0, 2 * np.pi, (h, w))
    e = np.stack([r * np.cos(th), r * np.sin(th)], axis=2).astype(np.float32)
    gt[100:180, 300:700] = 0.0
    gt[200:204, 10:90, 0] = 0.0
    flow = (gt - e).astype(np.float32)
    gt[30:40, 900:1000, 0] = 1e9
    gt[400:410, 5:50, 1] = -1e9
    return flow, gt


def test_metric_kernel_sintel_size_through_a_channel_sliced_padded_view():
    """Both flows of a [1,4,448,1024] stage-1-shaped tensor, read in place through the view's strides, cropped to rows 6:442."""
    from ssm_amd.flow_eval import flow_metric_sums
    from ssm_amd.frames import padded_dims
    (hp, wp), (top, left) = padded_dims(436, 1024)
    assert (hp, wp, top, left) == (448, 1024, 6, 0)
    cases = [sintel_sized_case(1), sintel_sized_case(2)]
    full = torch.full((1, 4, hp, wp), 1e6, dtype=torch.float32, device=DEV)          # the padding rows would wreck any sum that read them
    for c, (flow, _) in enumerate(cases):
        full[:, 2 * c:2 * c + 2, top:top + 436, left:left + 1024] = planar(flow[None])
    for c, (flow, gt) in enumerate(cases):
        for mode in (0, 1):
            sums = flow_metric_sums(full[:, 2 * c:2 * c + 2], T(gt[None]), top, left, mode).cpu().numpy()
            check_metric_sums(sums, flow[None], gt[None], mode)


def test_records_are_repeatable_and_independent_of_the_batch_and_stream():
    from ssm_amd.flow_eval import flow_metric_sums, flow_to_rgb
    rng = np.random.RandomState(6)
    flows = rng.uniform(-6, 6, (5, 83, 150, 2)).astype(np.float32)
    gts = rng.uniform(-6, 6, (5, 83, 150, 2)).astype(np.float32)
    fd, gd = planar(flows), T(gts)
    g_crop = gd[:, :79, :140].contiguous()                              # the cropped variants read rows 2.., columns 3.. of the flow
    for fn, g_use in ((lambda f, g: flow_metric_sums(f, g, 0, 0, 0), gd), (lambda f, g: flow_metric_sums(f, g, 2, 3, 1), g_crop),
                      (lambda f, g: flow_to_rgb(f, 80, 140, 1, 7), gd)):
        a = fn(fd, g_use).cpu()
        assert torch.equal(fn(fd, g_use).cpu(), a)
        for k in (0, 2, 4):
            assert torch.equal(fn(fd[k:k + 1], g_use[k:k + 1]).cpu()[0], a[k]), k
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            c = fn(fd, g_use)
        torch.cuda.current_stream().wait_stream(s)
        assert torch.equal(c.cpu(), a)


def test_colour_kernel_matches_the_reference_images(golden):
    from ssm_amd.flow_eval import flow_to_rgb
    g = golden("flow_eval")
    for k in range(N_COLOUR):
        flow, ref = g["c%d_flow" % k], g["c%d_image" % k]
        h, w = flow.shape[:2]
        got = flow_to_rgb(planar(flow[None]), h, w)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (1, h, w, 3)
        got = got.cpu().numpy()[0]
        diff = np.abs(got.astype(int) - ref.astype(int))
        print("colour field %d %s: %d of %d values differ from the reference, max %d level(s)" % (k, flow.shape, (diff > 0).sum(), diff.size, diff.max()))
        assert diff.max() <= 1, (k, np.argwhere(diff > 1)[:5])
        bad = (np.abs(flow) > 1e7).any(axis=2) | np.isnan(flow).any(axis=2)
        assert (got[bad] == 0).all(), k
        assert ((got == 0).all(axis=2) == (ref == 0).all(axis=2)).all(), k
    # a crop of a larger, channel-sliced tensor is the image of the cropped field
    flow, ref = g["c5_flow"], g["c5_image"]
    h, w = flow.shape[:2]
    full = torch.full((2, 4, h + 10, w + 16), 50.0, dtype=torch.float32, device=DEV)
    full[1, 2:4, 4:4 + h, 8:8 + w] = planar(flow[None])[0]
    got = flow_to_rgb(full[1:2, 2:4], h, w, 4, 8).cpu().numpy()[0]
    assert np.abs(got.astype(int) - ref.astype(int)).max() <= 1


def test_argument_checks():
    from ssm_amd.flow_eval import flow_metric_sums, flow_to_rgb
    f = torch.zeros(2, 2, 32, 40, device=DEV)
    g = torch.zeros(2, 32, 40, 2, device=DEV)
    with pytest.raises(RuntimeError, match="on the GPU"):
        flow_metric_sums(f.cpu(), g)
    with pytest.raises(RuntimeError, match="on the GPU"):
        flow_metric_sums(f, g.cpu())
    with pytest.raises(RuntimeError, match="float32"):
        flow_metric_sums(f.double(), g)
    with pytest.raises(RuntimeError, match=r"\[N,2,H,W\]"):
        flow_metric_sums(torch.zeros(2, 4, 32, 40, device=DEV), g)
    with pytest.raises(RuntimeError, match="differ"):
        flow_metric_sums(f[:1], g)
    with pytest.raises(RuntimeError, match="does not fit"):
        flow_metric_sums(f, g, 1, 0)
    with pytest.raises(RuntimeError, match="mode"):
        flow_metric_sums(f, g, 0, 0, 2)
    with pytest.raises(RuntimeError, match="does not fit"):
        flow_to_rgb(f, 32, 40, 0, 1)
    with pytest.raises(RuntimeError, match="on the GPU"):
        flow_to_rgb(f.cpu(), 32, 40)


@pytest.mark.parametrize("mode", ["f32w", "f32"])
def test_estimate_flow_is_bitwise_the_full_forward_stage1(golden, mode):
    from ssm_amd.weights import synthetic_frames
    cfg, m = make_model(mode)
    half = torch.full((1, 1, 1, 1, 1), 0.5, device=DEV)
    pair64 = torch.from_numpy(golden("stages_64")["pair"]).to(DEV)                      # [1,6,64,64]
    big = synthetic_frames(2, 448, 1024, seed=4).to(DEV)                                # [1,2,3,448,1024]
    for x in (pair64.view(1, 2, 3, 64, 64), big):
        before = m.interpolate(x, [0.25, 0.75]).clone()
        _, inter = m(x, half, inference_mode=True)
        flow = m.estimate_flow(x)
        assert flow.dtype == torch.float32 and tuple(flow.shape) == (1, 4) + tuple(x.shape[-2:]) and flow.is_contiguous()
        assert torch.equal(flow[:, 0:2], inter[0]) and torch.equal(flow[:, 2:4], inter[1])
        assert torch.equal(m.estimate_flow(x.reshape(1, 6, *x.shape[-2:])), flow)      # the [B,6,H,W] form
        planes = m.estimate_flow(x, want_planes=True)
        assert torch.equal(planes.interior, flow)
        assert torch.equal(m.interpolate(x, [0.25, 0.75]), before), "the flow plan and the pair engine clobber each other"
    two = torch.cat([pair64, pair64.flip(3)], 0)                                         # a batch: entry 0 is the single pair
    _, inter2 = m(two.view(2, 2, 3, 64, 64), half.expand(2, -1, -1, -1, -1), inference_mode=True)
    flow2 = m.estimate_flow(two)
    assert torch.equal(flow2[:, 0:2], inter2[0]) and torch.equal(flow2[:, 2:4], inter2[1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.estimate_flow(pair64.cpu())


def test_flow_evaluator_on_a_synthetic_clip():
    """5 frames of 60 x 90; ground truth = the model's own stage-1 flow plus (3, 4) on a rectangle: the error is 5 px there and 0
    elsewhere, so EPE = 5 * the rectangle's share (to the fp32 rounding of flow + 3 - flow) and the 3-px share is the share itself."""
    from ssm_amd.flow_eval import FlowEvaluator, clip_flow_samples
    from ssm_amd.frames import frames_from_u8
    from ssm_amd.weights import synthetic_frames_u8
    cfg, m = make_model()
    h, w = 60, 90
    clip = synthetic_frames_u8(5, h, w, seed=11).permute(0, 2, 3, 1).contiguous().to(DEV)
    x = frames_from_u8(clip, cfg, pad_before_norm=False)
    assert tuple(x.shape) == (5, 3, 64, 96)
    share = (20 * 30) / float(h * w)
    flows = []
    for i in range(4):
        own = m.estimate_flow(torch.stack([x[i], x[i + 1]])[None])[0, 0:2, 2:62, 3:93].permute(1, 2, 0).contiguous()
        own[10:30, 40:70, 0] += 3.0
        own[10:30, 40:70, 1] += 4.0
        flows.append(own)
    res, evs = {}, {}
    for mode in ("host", "device"):
        evs[mode] = FlowEvaluator(cfg, m, h, w, metrics=mode)
        res[mode] = evs[mode].run_evaluation(clip_flow_samples(clip, flows, cfg))
        assert res[mode]["samples"] == 4
        assert evs[mode].pct_error == [share] * 4, (mode, evs[mode].pct_error, share)
        np.testing.assert_allclose(evs[mode].EPE, [5.0 * share] * 4, rtol=1e-5, atol=0)
        assert all(type(v) is float for v in evs[mode].EPE + evs[mode].pct_error)
    np.testing.assert_allclose(evs["device"].EPE, evs["host"].EPE, rtol=2e-6, atol=0)
    assert evs["device"].pct_error == evs["host"].pct_error


def write_ini(tmp_path, root):
    from ssm_amd.config import CONFIG_DIR
    lines = open(os.path.join(CONFIG_DIR, "superslomo_original.ini")).read().splitlines()
    out, section = [], None
    for ln in lines:
        if ln.strip().startswith("["):
            section = ln.strip()
        if section == "[SINTEL_EPE_DATA]" and ln.split("=")[0].strip() == "ROOTDIR":
            ln = "ROOTDIR = %s" % root
        out.append(ln)
    p = tmp_path / "flow.ini"
    p.write_text("\n".join(out) + "\n")
    return str(p)


def test_flow_cli_on_a_sintel_shaped_tree(tmp_path, caplog):
    import logging
    caplog.set_level(logging.INFO)
    from PIL import Image
    import evaluate_optical_flow_results as S
    from utils.flo_utils import write_flow
    from ssm_amd.flow_eval import FlowEvaluator, clip_flow_samples
    from ssm_amd.weights import synthetic_frames_u8
    cfg, m = make_model()
    h, w = 60, 90
    root = tmp_path / "training"
    rng = np.random.RandomState(3)
    want = {"host": FlowEvaluator(cfg, m, h, w, metrics="host"), "device": FlowEvaluator(cfg, m, h, w, metrics="device")}
    for ci, (name, n) in enumerate((("alley_1", 4), ("bamboo_2", 3))):
        clip = synthetic_frames_u8(n, h, w, seed=20 + ci).permute(0, 2, 3, 1).contiguous()
        (root / "final" / name).mkdir(parents=True)
        (root / "flow" / name).mkdir(parents=True)
        flows = rng.uniform(-4, 4, (n - 1, h, w, 2)).astype(np.float32)
        for i in range(n):
            Image.fromarray(clip[i].numpy()).save(root / "final" / name / ("frame_%04d.png" % (i + 1)))
        for i in range(n - 1):
            write_flow(flows[i], str(root / "flow" / name / ("frame_%04d.flo" % (i + 1))))
        for ev in want.values():
            ev.run_evaluation(clip_flow_samples(clip.to(DEV), torch.from_numpy(flows), cfg))
    ini = write_ini(tmp_path, str(root))
    for mode in ("host", "device"):
        got = S.main(["-c", ini, "--log", str(tmp_path / "l.log"), "--metrics", mode], model=m)
        assert len(want[mode].EPE) == 5 and got == want[mode].means(), (mode, got, want[mode].means())
    assert "Final average: EPE: %.3f 3_pct_error: %.3f" % want["device"].means() in caplog.text and "So Far: EPE:" in caplog.text
    (root / "flow" / "alley_1" / "frame_0003.flo").unlink()                              # a training root checks images == flows + 1
    with pytest.raises(AssertionError, match="alley_1"):
        S.main(["-c", ini, "--log", str(tmp_path / "l.log")], model=m)


def test_visualize_cli_flow_png(tmp_path):
    from PIL import Image
    import visualize_interpolation as V
    from ssm_amd.config import CONFIG_DIR
    from ssm_amd.flow_eval import flow_to_rgb
    from ssm_amd.frames import frames_from_u8
    from ssm_amd.weights import synthetic_frames_u8
    cfg, m = make_model()
    clip = synthetic_frames_u8(3, 60, 90, seed=5).permute(0, 2, 3, 1).contiguous()
    src = tmp_path / "in"
    src.mkdir()
    for i in range(3):
        Image.fromarray(clip[i].numpy()).save(src / ("f_%03d.png" % i))
    base = ["-c", os.path.join(CONFIG_DIR, "superslomo_original.ini"), "--log", str(tmp_path / "l.log"), "--input_dir", str(src),
            "--img_type", "png", "--upsample_rate", "4", "--output_dir", str(tmp_path / "out")]
    assert V.main(base + ["--expt", "plain"], model=m) == 9
    assert sorted(os.listdir(tmp_path / "out" / "plain")) == ["images"]
    assert V.main(base + ["--expt", "npy", "--show_intermediate_outputs"], model=m) == 9
    assert sorted(os.listdir(tmp_path / "out" / "npy")) == ["images", "refined_flow", "visibility_map"]
    assert V.main(base + ["--expt", "plain2", "--flow_png"], model=m) == 9                # the flag alone writes nothing more
    assert sorted(os.listdir(tmp_path / "out" / "plain2")) == ["images"]
    assert V.main(base + ["--expt", "png", "--show_intermediate_outputs", "--flow_png"], model=m) == 9
    out = tmp_path / "out" / "png"
    assert sorted(os.listdir(out)) == ["estimated_flow_01", "estimated_flow_10", "images", "refined_flow", "refined_flow_t0",
                                       "refined_flow_t1", "visibility_map"]
    assert sorted(os.listdir(out / "refined_flow")) == sorted(os.listdir(tmp_path / "out" / "npy" / "refined_flow"))
    assert sorted(os.listdir(out / "estimated_flow_01")) == ["Flow_01_00004.png", "Flow_01_00008.png"]
    assert sorted(os.listdir(out / "estimated_flow_10")) == ["Flow_10_00004.png", "Flow_10_00008.png"]
    counts = [1, 2, 3, 5, 6, 7]
    assert sorted(os.listdir(out / "refined_flow_t1")) == ["flow_t1_%05d.png" % c for c in counts]
    assert sorted(os.listdir(out / "refined_flow_t0")) == ["flow_t0_%05d.png" % c for c in counts]
    # the same fields through flow_to_rgb
    x = frames_from_u8(clip.to(DEV), cfg, pad_before_norm=True)
    pair = torch.stack([x[1], x[2]])[None]
    _, inter = m(pair, torch.full((1, 1, 1, 1, 1), 0.5, device=DEV), inference_mode=True)
    for d, name, field in (("estimated_flow_01", "Flow_01_00008.png", inter[0]), ("estimated_flow_10", "Flow_10_00008.png", inter[1]),
                           ("refined_flow_t1", "flow_t1_00006.png", inter[4]), ("refined_flow_t0", "flow_t0_00006.png", inter[5])):
        want = flow_to_rgb(field, 60, 90, 2, 3)[0].cpu().numpy()
        got = np.asarray(Image.open(out / d / name))
        assert got.shape == (60, 90, 3) and np.array_equal(got, want), (d, name)
        assert got.std() > 1.0
