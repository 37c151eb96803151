"""The coarse-flow mode on the GPU (flow_scale = 2 | 4: U-Nets at 1/s of the frame's size, synthesis at full size; an
approximation of the reference's output, not parity).

  the kernel alone   ssm_synthesize_upscaled_fwd against the float64 evaluation of its definition (tests/coarse_refs.py).  Bar: with
                     d = max |float32 CPU evaluation of the same reference - float64| on the same inputs, the kernel must lie within
                     max(4 d, 1e-6): it performs the same rounded operations, the factor covers another valid order in the bilinear sums.
                     Measured on the MI355X, kernel distance / d (per-entry run; the sliced-view run gives the per-entry run's bits):
                       (h, w, s) = (3, 5, 2)    small 9.26e-07 / 1.48e-06   outside 9.64e-07 / 9.64e-07
                       (h, w, s) = (5, 33, 4)   small 2.31e-05 / 2.31e-05   outside 3.31e-05 / 3.31e-05
                       (h, w, s) = (7, 40, 2)   small 1.13e-05 / 1.13e-05   outside 1.60e-05 / 1.20e-05
                     and with one frame pair for all entries 1.06e-06 / 1.48e-06, 9.64e-07 / 9.64e-07, 2.20e-05 / 2.20e-05,
                     3.31e-05 / 3.31e-05, 1.39e-05 / 1.17e-05, 1.48e-05 / 1.21e-05: 0.63 to 1.33 d, against a bound of 4 d (the
                     frames are white noise: their gradients multiply the rounding of the sampling coordinates).  The engine's frames
                     lie 1.00 d from the float64 definition applied to its aux (d = 1.6e-5 ... 3.0e-5 at 128x128 and 128x256).
  the engine         CoarseFlowEngine == the pieces called by hand (ssm_avgpool2_fwd once or twice, a plain PairEngine at the low size,
                     the kernel on its aux), bit for bit, and within the kernel's bar of the float64 definition applied to that aux;
                     flow_scale=1 through every new keyword is the call without the keyword, bit for bit
  the video loop     a streamed clip at flow_scale=2 == ingest -> interpolate(flow_scale=2) -> egress per pair, byte for byte
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coarse_refs as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SHAPES = [(3, 5, 2), (5, 33, 4), (7, 40, 2)]          # (h, w, s): one block; two blocks along x with a ragged edge; two along y
TS = [0.25, 0.5, 0.75]


def hb():
    from ssm_amd import hipbind
    return hipbind


def run_kernel(img6, aux, t, y3, B, H, W, s, broadcast=False):
    h = hb()
    i6 = h.view_of(img6)
    if broadcast:
        i6.sb = 0
    h.check(h.load().ssm_synthesize_upscaled_fwd(i6, h.view_of(aux), t.data_ptr(), h.view_of(y3), B, H, W, s, h.stream_ptr()))
    torch.cuda.synchronize()


def assert_within(got, ref, what):
    want, d, bound = ref
    dist = (got.detach().cpu().double() - want).abs().max().item()
    msg = "%s: max |kernel - float64| = %.3e, d = max |float32 CPU - float64| = %.3e, bound max(4 d, 1e-6) = %.3e" % (what, dist, d, bound)
    print(msg)
    assert bool(torch.isfinite(got).all()) and dist <= bound, msg


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("h,w,s", SHAPES)
def test_kernel_against_float64(h, w, s, family):
    c = R.kernel_case(h, w, s, family)
    H, W, B = c["H"], c["W"], 3
    img6, aux, t = c["img6"].to(DEV), c["aux"].to(DEV), c["t"].to(DEV)
    tag = "(h,w,s)=(%d,%d,%d) %s" % (h, w, s, family)
    # one frame pair for every entry (sb = 0), then a pair per entry
    y = torch.full((B, 3, H, W), float("nan"), device=DEV)
    run_kernel(img6[:1], aux, t, y, B, H, W, s, broadcast=True)
    assert_within(y, c["bcast"], tag + " broadcast")
    y_each = torch.full((B, 3, H, W), float("nan"), device=DEV)
    run_kernel(img6, aux, t, y_each, B, H, W, s)
    assert_within(y_each, c["each"], tag + " per entry")
    assert torch.equal(y[0], y_each[0])
    # y3 and aux_lo as channel slices of larger tensors with padded rows: non-trivial sc and sh; what lies around them stays untouched
    big_y = torch.full((B, 5, H + 3, W + 5), -7.0, device=DEV)
    big_a = torch.full((B, 9, h + 2, w + 3), float("nan"), device=DEV)
    ys, as_ = big_y[:, 1:4, 2:2 + H, 3:3 + W], big_a[:, 2:7, 1:1 + h, 2:2 + w]
    as_.copy_(aux)
    run_kernel(img6, as_, t, ys, B, H, W, s)
    assert torch.equal(ys, y_each), "sliced views give other values than contiguous tensors"
    assert_within(ys, c["each"], tag + " sliced views")
    mask = torch.ones_like(big_y, dtype=torch.bool)
    mask[:, 1:4, 2:2 + H, 3:3 + W] = False
    assert bool((big_y[mask] == -7.0).all()), "the kernel wrote outside its y3 view"


def test_kernel_refuses_on_the_device_side_too():
    """The argument checks answer with tensors on the GPU as they do without (tests/test_coarse_cpu.py): nothing is launched."""
    h = hb()
    x = torch.zeros(1, 6, 8, 8, device=DEV)
    a = torch.zeros(1, 5, 4, 4, device=DEV)
    y = torch.zeros(1, 3, 8, 8, device=DEV)
    t = torch.full((1,), 0.5, device=DEV)
    with pytest.raises(RuntimeError, match="s must be 2 or 4"):
        h.check(h.load().ssm_synthesize_upscaled_fwd(h.view_of(x), h.view_of(a), t.data_ptr(), h.view_of(y), 1, 8, 8, 3, h.stream_ptr()))
    with pytest.raises(RuntimeError, match="multiples of s"):
        h.check(h.load().ssm_synthesize_upscaled_fwd(h.view_of(x), h.view_of(a), t.data_ptr(), h.view_of(y), 1, 6, 8, 4, h.stream_ptr()))


# ---- the engine ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    from models.superslomo_r import FullModel
    from ssm_amd.config import load_config, synthetic_weight_overrides
    from ssm_amd.weights import synthetic_state_dict
    cfg = load_config("superslomo_original.ini", synthetic_weight_overrides())
    m = FullModel(cfg)
    sd1, sd2 = synthetic_state_dict(1), synthetic_state_dict(2)
    m.stage1_model.load_state_dict(sd1)
    m.stage2_model.load_state_dict(sd2)
    m = m.to(DEV).eval()
    dsd = lambda mod: {k: v.detach() for k, v in mod.state_dict().items()}      # noqa: E731
    return cfg, m, dsd(m.stage1_model), dsd(m.stage2_model)


def pairs_of(P, H, W, seed=11):
    from ssm_amd.weights import synthetic_frames
    x = synthetic_frames(P + 1, H, W, seed=seed)[0].to(DEV)          # [P+1,3,H,W]
    return torch.cat([x[:-1], x[1:]], 1).contiguous()                # [P,6,H,W]


def by_hand(sd1, sd2, img6, t, s, mode):
    """The engine's pieces, called one by one: (frames [P*G,3,H,W], the low-resolution aux they were synthesised from)."""
    from ssm_amd.engine import PairEngine
    h = hb()
    lib, st = h.load(), h.stream_ptr()
    P, _, H, W = img6.shape
    G = t.numel()
    src = img6
    for _ in range(s.bit_length() - 1):
        dst = torch.empty(P, 6, src.shape[2] // 2, src.shape[3] // 2, device=DEV)
        h.check(lib.ssm_avgpool2_fwd(h.view_of(src), h.view_of(dst), P, 6, src.shape[2], src.shape[3], st))
        src = dst
    assert tuple(src.shape) == (P, 6, H // s, W // s)
    lo = PairEngine(sd1, sd2, P, P * G, H // s, W // s, DEV, True, mode)
    lo.run(src, t, want_aux=True)
    aux = lo.aux.clone()
    tt = t.repeat(P)
    out = torch.full((P * G, 3, H, W), float("nan"), device=DEV)
    for p in range(P):
        run_kernel(img6[p:p + 1], aux[p * G:(p + 1) * G], tt[p * G:(p + 1) * G], out[p * G:(p + 1) * G], G, H, W, s, broadcast=True)
    return out, aux, tt


@pytest.mark.parametrize("H,W,s,P", [(128, 128, 2, 1), (128, 128, 2, 2), (128, 256, 4, 1), (128, 256, 4, 2)])
def test_engine_is_its_pieces_and_meets_the_kernel_bar(model, H, W, s, P):
    from ssm_amd.engine import CoarseFlowEngine
    cfg, m, sd1, sd2 = model
    mode = "f32w"
    img6 = pairs_of(P, H, W)
    t = torch.tensor(TS, device=DEV)
    want, aux, tt = by_hand(sd1, sd2, img6, t, s, mode)
    eng = CoarseFlowEngine(sd1, sd2, P, len(TS), H, W, DEV, s, True, mode)
    got = eng.run(img6, t)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (P * len(TS), 3, H, W) and torch.equal(got, want), "engine != avgpool -> PairEngine -> upscaled synthesis by hand"
    assert torch.equal(eng.lo.aux, aux)
    inter = eng.intermediates()
    assert len(inter) == 7 and tuple(inter[4].shape) == (P * len(TS), 2, H // s, W // s) and torch.equal(inter[6], aux[:, 4:5])
    # ... and the frames are the float64 definition applied to that aux, to the kernel's own bar
    G = len(TS)
    for p in range(P):
        sl = slice(p * G, (p + 1) * G)
        assert_within(got[sl], R.bar(img6[p:p + 1], aux[sl], tt[sl], s), "engine %dx%d s=%d pair %d/%d" % (H, W, s, p, P))
    # the public surface reaches the same engine: interpolate (one pair) and interpolate_many (a PairPipeline, P pairs per pass)
    m.precision = mode
    try:
        one = m.interpolate(img6[:1].view(1, 2, 3, H, W), TS, flow_scale=s)
        if P == 1:
            assert torch.equal(one, want)
        many = m.interpolate_many([img6[p:p + 1].view(1, 2, 3, H, W) for p in range(P)], TS, n_streams=2, pairs_per_batch=P, flow_scale=s)
        assert len(many) == P and torch.equal(torch.cat(many, 0), want)          # (a pass of P pairs plans its convolutions for that batch:
        assert tuple(one.shape) == tuple(many[0].shape)                         # equal to the one-pair engine's frames only at P = 1)
    finally:
        m.precision = None

def test_sizes_are_refused_by_rule(model):
    cfg, m, sd1, sd2 = model
    x = torch.zeros(1, 2, 3, 96, 128, device=DEV)
    with pytest.raises(AssertionError, match=r"multiples of 32\*flow_scale = 64"):
        m.interpolate(x, TS, flow_scale=2)
    with pytest.raises(ValueError, match="flow_scale must be 1, 2 or 4"):
        m.interpolate(x, TS, flow_scale=3)


def test_flow_scale_one_is_the_call_without_the_keyword(model, tmp_path):
    from ssm_amd import video as V
    from ssm_amd.engine import PairEngine, PairPipeline
    from ssm_amd.frames import frames_from_u8
    from ssm_amd.weights import synthetic_frames_u8
    cfg, m, sd1, sd2 = model
    H = W = 64
    img6 = pairs_of(2, H, W, seed=3)
    pair = img6[:1].view(1, 2, 3, H, W)
    a = m.interpolate(pair, TS)
    b = m.interpolate(pair, TS, flow_scale=1)
    assert torch.equal(a, b) and isinstance(m._engine[1], PairEngine)
    prs = [img6[p:p + 1].view(1, 2, 3, H, W) for p in range(2)]
    a = m.interpolate_many(prs, TS)
    b = m.interpolate_many(prs, TS, flow_scale=1)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    t = torch.tensor(TS, device=DEV)
    outs = []
    for kw in ({}, {"flow_scale": 1}):
        pipe = PairPipeline(sd1, sd2, len(TS), H, W, DEV, True, "f32w", n_streams=1, **kw)
        assert all(type(e) is PairEngine for e in pipe.engines)
        outs.append(pipe.submit(img6[:1], t, clone=True))
        pipe.sync()
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])
    # ingest keywords: multiple=32 is the default canvas
    u8 = synthetic_frames_u8(2, 46, 70, seed=2).permute(0, 2, 3, 1).contiguous().to(DEV)
    assert torch.equal(frames_from_u8(u8, cfg, True), frames_from_u8(u8, cfg, True, multiple=32))
    h, w, n, rate = 46, 70, 4, 4
    payloads = clip_payloads(n, h, w)
    dev = torch.from_numpy(payloads).to(DEV)
    assert torch.equal(V.frames_from_yuv(dev, h, w), V.frames_from_yuv(dev, h, w, multiple=32))
    got = []
    for i, kw in enumerate(({}, {"flow_scale": 1})):
        got.append(stream_clip(m, cfg, payloads, h, w, rate, tmp_path / ("f%d" % i), **kw))
    assert np.array_equal(got[0], got[1])


# ---- the video loop --------------------------------------------------------------------------------------------------------------------
def clip_payloads(n, h, w, seed=5):
    """A moving synthetic 4:2:0 clip as Y4M payloads [n, frame_bytes] uint8 (legal limited-range codes, through the yardstick's egress)."""
    from ssm_amd import video as V
    from ssm_amd.weights import IMAGENET_MEAN, IMAGENET_STD, synthetic_frames_u8
    rgb = synthetic_frames_u8(n, h, w, seed=seed).numpy().astype(np.float32) / np.float32(255.0)
    x = (rgb - np.float32(IMAGENET_MEAN)[None, :, None, None]) / np.float32(IMAGENET_STD)[None, :, None, None]
    return V.frames_to_yuv_host(x, h, w, V.CENTRED, V.default_matrix(h), V.LIMITED)


def stream_clip(m, cfg, payloads, h, w, rate, tmp, **kw):
    from ssm_amd import video as V
    os.makedirs(str(tmp), exist_ok=True)
    src, dst = os.path.join(str(tmp), "in.y4m"), os.path.join(str(tmp), "out.y4m")
    with V.Y4MWriter(src, w, h, rate=(30, 1), aspect=(1, 1), chroma="420jpeg") as wr:
        for p in payloads:
            wr.write_frame(p)
    vi = V.VideoInterpolator(m, cfg, upsample_rate=rate, n_streams=2, **kw)
    with V.Y4MReader(src) as r, V.Y4MWriter.like(dst, r, rate=V.output_rate(r.rate, rate)) as wr:
        count = vi.run(r, wr)
    assert count == (len(payloads) - 1) * rate + 1
    with V.Y4MReader(dst) as r:
        frames, buf = [], np.empty(r.frame_bytes, np.uint8)
        while r.read_frame_into(buf):
            frames.append(buf.copy())
    assert len(frames) == count
    return np.stack(frames)


def test_streamed_clip_at_flow_scale_2_equals_per_pair_evaluation(model, tmp_path):
    """6 frames of 96x160 4:2:0 on the 128x192 canvas of flow_scale=2."""
    from ssm_amd import video as V
    from ssm_amd.evaluation import t_values
    cfg, m, _, _ = model
    h, w, n, rate, s = 96, 160, 6, 4, 2
    payloads = clip_payloads(n, h, w)
    assert V.VideoInterpolator(m, cfg, upsample_rate=rate, flow_scale=s).canvas(h, w) == (128, 192)
    got = stream_clip(m, cfg, payloads, h, w, rate, tmp_path, flow_scale=s)
    assert np.array_equal(got[::rate], payloads), "original frames must pass through as their own bytes"
    matrix, crange = V.default_matrix(h), V.LIMITED
    dev = torch.from_numpy(payloads).to(DEV)
    want = [payloads[0]]
    for i in range(n - 1):
        x = V.frames_from_yuv(dev[i:i + 2], h, w, V.CENTRED, matrix, crange, cfg, True, multiple=32 * s)
        assert tuple(x.shape) == (2, 3, 128, 192)
        frames = m.interpolate(x[None], t_values(rate), flow_scale=s)
        want.extend(V.frames_to_yuv(frames, h, w, V.CENTRED, matrix, crange, cfg).cpu().numpy())
        want.append(payloads[i + 1])
    want = np.stack(want)
    assert np.array_equal(got, want), int((got != want).sum())
    # and the mode is not the default one in disguise: the default canvas is 96x160 and its frames differ
    base = stream_clip(m, cfg, payloads, h, w, rate, tmp_path / "base")
    assert base.shape == got.shape and not np.array_equal(base, got)
