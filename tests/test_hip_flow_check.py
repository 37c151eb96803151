"""Forward-backward flow consistency on the GPU: ssm_flow_consistency_fwd against its numpy yardstick
(ssm_amd.flow_eval.flow_consistency_host) - the counts and the mask word for word, the residual sum within 1e-12 relative, the bar of the
EPE sum - and VideoInterpolator(flow_check=) on small synthetic clips: the report changes no byte, `flow_checks` is the yardstick on the
flows FullModel.estimate_flow gives for the same frames, and a threshold replaces exactly the pairs at or above it by the nearer input
frame's bytes, the scene-cut rule.

With the synthetic weights the scores are whatever they are: nothing here reads them as quality."""
import io
import os
import sys
from fractions import Fraction as Fr

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import video_cut_clips as C  # noqa: E402
from video_clips import V, clip_payloads, deep_payloads, frames_of, synthetic_model, y4m  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
REL = 1e-12          # the residual sum: fp64 sums of the same fp32 terms in two orders
POISON = 0xAB


def FE():
    from ssm_amd import flow_eval
    return flow_eval


# ---- the kernel ---------------------------------------------------------------------------------------------------------------------------
CROPS = ((1, 1), (3, 5), (8, 8), (37, 70), (50, 200))          # 50 x 200 = 10000 pixels: five workspace slots of 2048
TOP, LEFT, PLANES = 2, 3, 6          # the crop's origin in the view; planes per batch entry of the buffer, four of them the flow's


def fields(n, h, w, seed=0, reach=6.0):
    """[n,4,h,w] float32: F01 a motion of up to `reach` pixels per field under +-0.7 px of grain, F10 its negative under grain of its own -
    so that F + G' is the grain's, around the threshold's 0.5 px^2: consistent, inconsistent and leaving pixels all occur on a crop that
    has room for them."""
    rng = np.random.RandomState(1000 * h + w + seed)
    c = rng.uniform(-reach, reach, size=(n, 2, 1, 1))
    f01 = c + rng.uniform(-0.7, 0.7, size=(n, 2, h, w))
    f10 = -c + rng.uniform(-0.7, 0.7, size=(n, 2, h, w))
    return np.concatenate([f01, f10], axis=1).astype(np.float32)


def in_view(flow4):
    """The fields inside a larger buffer [n, PLANES, h + 5, w + 7] that is NaN everywhere else - the canvas around the crop, and two planes
    behind the flow's four, so the view's batch stride is larger than the entry: (the buffer, its first four planes as the kernel's view)."""
    n, _, h, w = flow4.shape
    buf = np.full((n, PLANES, h + 5, w + 7), np.nan, np.float32)
    buf[:, :4, TOP:TOP + h, LEFT:LEFT + w] = flow4
    return buf


def device_call(buf, h, w, alpha, beta, want_mask=True, top=TOP, left=LEFT):
    """ssm_flow_consistency_fwd through the library on planes [:4] of `buf`: (record [n,2,4] float64, mask [n,2,h,w] uint8 or None).  The
    mask lies inside a poisoned buffer with 32 bytes of slack on either side, which must come back untouched."""
    from ssm_amd import hipbind as hb
    lib = hb.load()
    t = torch.from_numpy(buf).to(DEV)
    view = t[:, :4]
    n = buf.shape[0]
    assert view.stride(0) == buf.shape[1] * buf.shape[2] * buf.shape[3], "the batch stride is the buffer's, not four planes"
    ws = torch.empty(lib.ssm_flow_consistency_workspace_bytes(n, h, w), dtype=torch.uint8, device=DEV)
    out = torch.full((n, 2, 4), -1.0, dtype=torch.float64, device=DEV)
    size = n * 2 * h * w
    mbuf = torch.full((size + 64,), POISON, dtype=torch.uint8, device=DEV)
    hb.check(lib.ssm_flow_consistency_fwd(hb.view_of(view), n, h, w, top, left, alpha, beta, ws.data_ptr(), out.data_ptr(),
                                          mbuf.data_ptr() + 32 if want_mask else None, hb.stream_ptr()))
    torch.cuda.synchronize()
    m = mbuf.cpu().numpy()
    assert (m[:32] == POISON).all() and (m[32 + size:] == POISON).all(), "the slack around the mask"
    if not want_mask:
        assert (m == POISON).all()
    return out.cpu().numpy(), m[32:32 + size].reshape(n, 2, h, w) if want_mask else None


def agree(got, want):
    """Counts word for word, the residual sums within REL."""
    assert np.array_equal(got[..., :3], want[..., :3]), (got[..., :3], want[..., :3])
    assert np.all(np.abs(got[..., 3] - want[..., 3]) <= REL * np.abs(want[..., 3])), (got[..., 3], want[..., 3])


_refs = {}


def reference(n, h, w):
    """(the buffer, the yardstick's record and mask) of a case, computed once."""
    if (n, h, w) not in _refs:
        buf = in_view(fields(n, h, w))
        _refs[n, h, w] = (buf,) + FE().flow_consistency_host(buf[:, :4], TOP, LEFT, h, w, FE().FLOW_ALPHA, FE().FLOW_BETA)
    return _refs[n, h, w]


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("h,w", CROPS)
def test_kernel_equals_its_yardstick(h, w, n):
    """The crop at (2, 3) of a view whose surround is NaN and whose batch stride is six planes: a tap outside the crop would show."""
    fe = FE()
    buf, want, want_mask = reference(n, h, w)
    assert (want[..., 0] + want[..., 2] == h * w).all()
    if h * w >= 2048:
        assert all((want_mask == s).any() for s in (0, 1, 2)), "every state occurs"
    got, mask = device_call(buf, h, w, fe.FLOW_ALPHA, fe.FLOW_BETA)
    agree(got, want)
    assert np.array_equal(mask, want_mask)
    again, no_mask = device_call(buf, h, w, fe.FLOW_ALPHA, fe.FLOW_BETA, want_mask=False)
    assert no_mask is None and again.tobytes() == got.tobytes(), "mask = null gives the same record, and two calls the same bits"


def test_a_pair_does_not_depend_on_its_batch():
    buf, _, _ = reference(3, 37, 70)
    fe = FE()
    whole, mask = device_call(buf, 37, 70, fe.FLOW_ALPHA, fe.FLOW_BETA)
    for k in range(3):
        one, m1 = device_call(buf[k:k + 1], 37, 70, fe.FLOW_ALPHA, fe.FLOW_BETA)
        assert one.tobytes() == whole[k:k + 1].tobytes() and np.array_equal(m1[0], mask[k])


def test_the_python_call_on_tensor_and_planes():
    """flow_eval.flow_consistency on a strided tensor, and on the padded planes of hipbind.Planes where stage 1 would leave them."""
    from ssm_amd import hipbind as hb
    fe = FE()
    buf, want, want_mask = reference(3, 37, 70)
    t = torch.from_numpy(buf).to(DEV)
    rec, mask = fe.flow_consistency(t[:, :4], 37, 70, TOP, LEFT, want_mask=True)
    agree(rec.cpu().numpy(), want)
    assert np.array_equal(mask.cpu().numpy(), want_mask)
    planes = hb.Planes(3, 4, buf.shape[2], buf.shape[3], DEV)
    planes.load(t[:, :4].contiguous())
    agree(fe.flow_consistency(planes, 37, 70, TOP, LEFT).cpu().numpy(), want)
    checks = [fe.FlowCheck.of(r) for r in rec.cpu().numpy()]
    assert [c.judged for c in checks] == [tuple(int(x) for x in r[:, 0]) for r in want]
    with pytest.raises(RuntimeError, match="does not fit"):
        fe.flow_consistency(t[:, :4], 37, 70, TOP + 4, LEFT)
    with pytest.raises(RuntimeError, match="four planes"):
        fe.flow_consistency(t[:, :2], 37, 70, TOP, LEFT)


def constant(h, w, f01, f10):
    x = np.empty((1, 4, h, w), np.float32)
    x[0, 0], x[0, 1], x[0, 2], x[0, 3] = f01[0], f01[1], f10[0], f10[1]
    return x


@pytest.mark.parametrize("f", [(2.0, -1.0), (0.5, 0.25)])
def test_closed_form_constant_fields(f):
    """F01 = f, F10 = -f on 6 x 9: nothing is inconsistent, every residual is 0; a pixel leaves iff x + u or y + v falls outside the crop."""
    h, w = 6, 9
    x = constant(h, w, f, (-f[0], -f[1]))
    got, mask = device_call(in_view(x), h, w, 0.01, 0.5)
    for d, (u, v) in enumerate((f, (-f[0], -f[1]))):
        stay = sum(1 for yy in range(h) for xx in range(w) if 0 <= xx + u <= w - 1 and 0 <= yy + v <= h - 1)
        assert got[0, d].tolist() == [stay, 0, h * w - stay, 0.0]
        assert (mask[0, d] == 2).sum() == h * w - stay and (mask[0, d] == 1).sum() == 0


def test_the_strict_edge():
    """alpha = 0, F01 = (2, 0), F10 = (-1, 0): e2 = 1 at every judged pixel.  beta = 1 judges nothing inconsistent, the float below 1 all."""
    h, w = 6, 9
    buf = in_view(constant(h, w, (2.0, 0.0), (-1.0, 0.0)))
    at, _ = device_call(buf, h, w, 0.0, 1.0)
    below, _ = device_call(buf, h, w, 0.0, float(np.nextafter(np.float32(1), np.float32(0))))
    assert at[0, :, 0].tolist() == [h * (w - 2), h * (w - 1)] == below[0, :, 0].tolist()
    assert at[0, :, 1].tolist() == [0, 0] and below[0, :, 1].tolist() == below[0, :, 0].tolist()
    assert at[0, :, 3].tolist() == [float(h * (w - 2)), float(h * (w - 1))], "every residual is 1"


def test_nan_and_inf_flows_leave():
    h, w = 8, 8
    x = fields(1, h, w, reach=0.5)
    x[0, 0, 1, 1], x[0, 1, 2, 2], x[0, 0, 3, 3], x[0, 2, 4, 4] = np.nan, np.inf, -np.inf, np.nan
    buf = in_view(x)
    want, want_mask = FE().flow_consistency_host(buf[:, :4], TOP, LEFT, h, w, 0.01, 0.5)
    got, mask = device_call(buf, h, w, 0.01, 0.5)
    assert np.array_equal(mask, want_mask) and mask[0, 0, 1, 1] == mask[0, 0, 2, 2] == mask[0, 0, 3, 3] == mask[0, 1, 4, 4] == 2
    assert np.array_equal(got[..., :3], want[..., :3])


# ---- the streamed loop ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    return synthetic_model(DEV)


# size, frames, colour-space tag, the run.  45 x 71 pads to 64 x 96: the picture sits at (9, 12) of the canvas.  Six frames at two pairs a
# pass: the last pass is short.  The timeline runs 240 -> 600 frames/s, step 2/5: every pair runs.
LEGS = {
    "rate2_pb1": ((45, 71), 5, "420jpeg", dict(upsample_rate=2, pairs_per_batch=1)),
    "rate3_pb2": ((45, 71), 6, "420jpeg", dict(upsample_rate=3, pairs_per_batch=2)),
    "timeline": ((64, 96), 5, "420jpeg", dict(target_rate=(600, 1), pairs_per_batch=1)),
    "422p10": ((64, 96), 4, "422p10", dict(upsample_rate=2, pairs_per_batch=2)),
}
IN_RATE = (240, 1)          # video_clips.y4m's


def stream(model, payloads, h, w, tag, **kw):
    """The clip through VideoInterpolator(**kw): (its frames, the interpolator)."""
    cfg, m = model
    v = V()
    r = v.Y4MReader(y4m(payloads, h, w, tag), extended=True)
    sink = io.BytesIO()
    wr = v.Y4MWriter.like(sink, r, rate=kw.get("target_rate") or r.rate)
    vi = v.VideoInterpolator(m, cfg, n_streams=2, **kw)
    count = vi.run(r, wr)
    got = frames_of(sink.getvalue())
    assert got.shape[0] == count == wr.frames_written
    return got, vi


def outputs_of(n, kw):
    """[(i, t)] of every output frame of an n-frame clip; t = 0: input frame i itself."""
    v = V()
    if "target_rate" in kw:
        return v.Timeline(v.timeline_step(IN_RATE, kw["target_rate"])).outputs(n)
    rate = kw["upsample_rate"]
    return [(k // rate, Fr(k % rate, rate)) for k in range((n - 1) * rate + 1)]


def with_fallback(plain, payloads, outputs, replaced):
    """The run without the option with every synthesised frame of the pairs in `replaced` exchanged for the nearer input frame's bytes."""
    want = plain.copy()
    for k, (i, t) in enumerate(outputs):
        if t > 0 and i in replaced:
            want[k] = payloads[i] if t < Fr(1, 2) else payloads[i + 1]
    return want


def yardstick_checks(model, payloads, h, w, tag, pairs, pb):
    """[(i, FlowCheck)] of the pairs by the yardstick, on the flows FullModel.estimate_flow gives for the frames as the loop ingests them,
    `pb` pairs a call as the loop's passes take them (a short last pass is filled with its last frame)."""
    cfg, m = model
    v, fe = V(), FE()
    layout, bits = v.EXTENDED_TAGS[tag]
    planes = v.frames_from_yuv(torch.from_numpy(payloads).to(DEV), h, w, layout, v.default_matrix(h), v.LIMITED, cfg, True, bits=bits)
    top, left = (planes.shape[2] - h) // 2, (planes.shape[3] - w) // 2
    out = []
    for p0 in range(0, len(pairs), pb):
        group = pairs[p0:p0 + pb]
        sides = [(i, i + 1) for i in group] + [(group[-1] + 1, group[-1] + 1)] * (pb - len(group))
        x = torch.stack([torch.stack([planes[a], planes[b]]) for a, b in sides])
        flow = m.estimate_flow(x).cpu().numpy()
        record, _ = fe.flow_consistency_host(flow, top, left, h, w, fe.FLOW_ALPHA, fe.FLOW_BETA)
        out += [(i, fe.FlowCheck.of(record[p])) for p, i in enumerate(group)]
    return out


def test_full_model_call_and_the_visualiser_masks(model, tmp_path):
    """FullModel.flow_consistency on a 60 x 90 picture inside its 64 x 96 canvas equals the yardstick on estimate_flow's fields, and
    visualize_interpolation.py --consistency_png writes that pair's two masks as grey 0 / 255 / 128 beside the flow maps."""
    from PIL import Image
    import visualize_interpolation as VI
    from ssm_amd.config import CONFIG_DIR
    from ssm_amd.frames import frames_from_u8
    from ssm_amd.weights import synthetic_frames_u8
    cfg, m = model
    fe = FE()
    h, w = 60, 90
    clip = synthetic_frames_u8(3, h, w, seed=5).permute(0, 2, 3, 1).contiguous()
    x = frames_from_u8(clip.to(DEV), cfg, pad_before_norm=True)
    pairs = torch.stack([torch.stack([x[0], x[1]]), torch.stack([x[1], x[2]])])
    top, left = (x.shape[2] - h) // 2, (x.shape[3] - w) // 2
    want, want_mask = fe.flow_consistency_host(m.estimate_flow(pairs).cpu().numpy(), top, left, h, w, fe.FLOW_ALPHA, fe.FLOW_BETA)
    checks, mask = m.flow_consistency(pairs, size=(h, w), want_mask=True)
    assert np.array_equal(mask.cpu().numpy(), want_mask)
    for c, r in zip(checks, want):
        ref = fe.FlowCheck.of(r)
        assert c[:3] == ref[:3] and all(abs(a - b) <= REL * abs(b) for a, b in zip(c.residual_sum, ref.residual_sum))
    assert m.flow_consistency(pairs, size=(h, w)) == checks
    src = tmp_path / "in"
    src.mkdir()
    for i in range(3):
        Image.fromarray(clip[i].numpy()).save(src / ("f_%03d.png" % i))
    argv = ["-c", os.path.join(CONFIG_DIR, "superslomo_original.ini"), "--log", str(tmp_path / "l.log"), "--input_dir", str(src),
            "--img_type", "png", "--upsample_rate", "2", "--output_dir", str(tmp_path / "out"), "--expt", "fb",
            "--show_intermediate_outputs", "--consistency_png"]
    assert VI.main(argv, model=m) == 5
    out = tmp_path / "out" / "fb"
    assert sorted(os.listdir(out)) == ["flow_consistency_01", "flow_consistency_10", "images", "refined_flow", "visibility_map"]
    grey = np.array([0, 255, 128], np.uint8)
    for d, name in enumerate(("01", "10")):
        assert sorted(os.listdir(out / ("flow_consistency_" + name))) == ["Consistency_%s_%05d.png" % (name, c) for c in (2, 4)]
        for k, c in enumerate((2, 4)):
            got = np.asarray(Image.open(out / ("flow_consistency_" + name) / ("Consistency_%s_%05d.png" % (name, c))))
            _, alone = fe.flow_consistency_host(m.estimate_flow(pairs[k:k + 1]).cpu().numpy(), top, left, h, w, fe.FLOW_ALPHA, fe.FLOW_BETA)
            assert np.array_equal(got, grey[alone[0, d]])          # the visualiser runs a pair at a time


_runs = {}


def leg(model, name):
    """What every test of a leg shares, run once: the payloads, the outputs' (i, t), the run without the option, the run with the report."""
    if name not in _runs:
        (h, w), n, tag, kw = LEGS[name]
        payloads = deep_payloads(n, h, w, tag)
        plain, vi0 = stream(model, payloads, h, w, tag, **kw)
        assert vi0.flow_checks == [] and vi0.flow_failed == []
        report, vi = stream(model, payloads, h, w, tag, flow_check=True, **kw)
        _runs[name] = (payloads, outputs_of(n, kw), plain, report, vi.flow_checks, vi.flow_failed)
    return _runs[name]


@pytest.mark.parametrize("name", sorted(LEGS))
def test_the_report_changes_no_byte_and_equals_the_yardstick(model, name):
    (h, w), n, tag, kw = LEGS[name]
    payloads, outputs, plain, report, checks, failed = leg(model, name)
    assert np.array_equal(report, plain) and failed == []
    ran = sorted({i for i, t in outputs if t > 0})
    assert [i for i, _ in checks] == ran == list(range(n - 1))
    want = yardstick_checks(model, payloads, h, w, tag, ran, kw["pairs_per_batch"])
    print(name, "scores", [(i, str(c.score), "%.4f" % c.mean_residual) for i, c in checks])
    for (i, got), (j, ref) in zip(checks, want):
        assert i == j and got[:3] == ref[:3], (i, got, ref)
        assert all(abs(a - b) <= REL * abs(b) for a, b in zip(got.residual_sum, ref.residual_sum)), (i, got, ref)
        assert all(jd + lv == h * w for jd, lv in zip(got.judged, got.leaves))


@pytest.mark.parametrize("name", sorted(LEGS))
def test_thresholds(model, name):
    """T = 2, above every score: the run without the option.  T = 0, which every score reaches: every pair that ran - so every pair with
    an inconsistent pixel - falls back.  T between two of the measured scores, where they are not all equal: exactly the pairs at or
    above it."""
    (h, w), n, tag, kw = LEGS[name]
    payloads, outputs, plain, _, checks, _ = leg(model, name)
    got, vi = stream(model, payloads, h, w, tag, flow_check=2, **kw)
    assert np.array_equal(got, plain) and vi.flow_failed == [] and vi.flow_checks == checks
    got, vi = stream(model, payloads, h, w, tag, flow_check=0, **kw)
    assert vi.flow_checks == checks == vi.flow_failed
    want = with_fallback(plain, payloads, outputs, {i for i, _ in checks})
    assert np.array_equal(got, want), int((got != want).sum())
    assert not np.array_equal(got, plain), "the synthesised frames are no input frames' bytes"
    scores = sorted({c.score for _, c in checks})
    if len(scores) > 1:
        t = (scores[(len(scores) - 1) // 2] + scores[(len(scores) - 1) // 2 + 1]) / 2
        got, vi = stream(model, payloads, h, w, tag, flow_check=t, **kw)
        fail = [(i, c) for i, c in checks if c.score >= t]
        assert 0 < len(fail) < len(checks) and vi.flow_failed == fail
        want = with_fallback(plain, payloads, outputs, {i for i, _ in fail})
        assert np.array_equal(got, want), int((got != want).sum())


def test_a_pair_falls_back_if_it_is_a_cut_or_fails_the_check(model):
    """The scene-cut clip on the fixed grid with both options: the cut pair and the pairs at or above T are replaced, both logs are kept."""
    h, w = C.SIZES[1]
    payloads = C.cut_clip(h, w)
    kw = dict(upsample_rate=2, pairs_per_batch=2)
    outputs = outputs_of(C.N_FRAMES, kw)
    plain, _ = stream(model, payloads, h, w, "420jpeg", **kw)
    _, vi = stream(model, payloads, h, w, "420jpeg", flow_check=True, **kw)
    scores = sorted({c.score for _, c in vi.flow_checks})
    t = scores[-1] if len(scores) > 1 else Fr(2)          # the worst pairs alone; with equal scores none, and the cut stands alone
    fail = [(i, c) for i, c in vi.flow_checks if c.score >= t]
    got, both = stream(model, payloads, h, w, "420jpeg", flow_check=t, scene_cut=C.THRESHOLD, **kw)
    assert both.cuts == [(C.CUT, C.pair_scores(payloads, h, w)[C.CUT][2])] and both.flow_failed == fail and both.flow_checks == vi.flow_checks
    want = with_fallback(plain, payloads, outputs, {C.CUT} | {i for i, _ in fail})
    assert np.array_equal(got, want), int((got != want).sum())
    assert np.array_equal(got[2 * C.CUT + 1], payloads[C.CUT + 1]) and not np.array_equal(plain[2 * C.CUT + 1], payloads[C.CUT + 1])
