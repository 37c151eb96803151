"""4:2:2 and 9- to 16-bit video on the GPU: ssm_frames_from_yuvx_fwd / ssm_frames_to_yuvx_fwd (csrc/ssm_video.hip) against their numpy
float32 yardsticks (ssm_amd.video.yuv_to_frames_host / frames_to_yuv_host with layout 3 and bits > 8, themselves held to a float64
evaluation in tests/test_video_deep_cpu.py) - BIT-equal planes and BYTE-equal codes, as tests/test_hip_video.py holds the 8-bit entry
points - against those entry points where both apply, and the streamed loop on the new formats against a pair-by-pair evaluation of the
same kernels."""
import io
import itertools
import os
import sys
from fractions import Fraction as Fr

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import video_deep_clips as D  # noqa: E402
from video_clips import V, read_clip  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SIZES = ((46, 70), (45, 71), (64, 96))          # even, odd (offsets 9/13 and 9/12 in the 64 x 96 canvas), and a canvas-filling size
FORMATS = [(lay, bits) for bits in (10, 16) for lay in (0, 1, 2, 3)] + [(3, 8)]


def egress_input(rng, n, h, w):
    """Planes denormalised about -0.55 .. 1.55 with the six saturating patches of tests/test_hip_video.py: both bounds of every plane."""
    hp, wp = -(-h // 32) * 32, -(-w // 32) * 32
    x = rng.uniform(-4.5, 5.0, size=(n, 3, hp, wp)).astype(np.float32)
    for i, rgb in enumerate(D.SATURATING):
        x[:, :, hp // 2 - 2:hp // 2 + 2, wp // 2 - 12 + 4 * i:wp // 2 - 8 + 4 * i] = np.where(np.float32(rgb) > 0, np.float32(5.0), np.float32(-4.5))[None, :, None, None]
    return x


def words(payload, bits):
    return payload if bits == 8 else payload.view("<u2")


@pytest.mark.parametrize("fmt,matrix,crange", list(itertools.product(FORMATS, (0, 1), (0, 1))))
def test_kernels_equal_their_yardsticks(fmt, matrix, crange):
    v = V()
    layout, bits = fmt
    seed = 10000 * bits + 1000 * layout + 100 * matrix + 10 * crange
    for (h, w), n, pbn in itertools.product(SIZES, (1, 3), (True, False)):
        payload = D.seeded_payload(n, h, w, layout, bits, seed + n)
        got = v.frames_from_yuv(torch.from_numpy(payload).to(DEV), h, w, layout, matrix, crange, None, pbn, bits=bits).cpu().numpy()
        want = v.yuv_to_frames_host(payload, h, w, layout, matrix, crange, pad_before_norm=pbn, bits=bits)
        assert got.shape == want.shape
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), \
            ("ingest", h, w, n, pbn, float(np.abs(got - want).max()), int((got != want).sum()))
    k = D.consts64(matrix, crange, bits)
    for (h, w), n in itertools.product(SIZES, (1, 3)):
        x = egress_input(np.random.RandomState(7 + seed + n), n, h, w)
        got = v.frames_to_yuv(torch.from_numpy(x).to(DEV), h, w, layout, matrix, crange, bits=bits).cpu().numpy()
        want = v.frames_to_yuv_host(x, h, w, layout, matrix, crange, bits=bits)
        ww = words(want, bits)
        assert ww[:, :h * w].min() == k["ylo"] and ww[:, :h * w].max() == k["yhi"] and ww[:, h * w:].min() == k["clo"] and \
            ww[:, h * w:].max() == k["chi"], "the expected codes reach both bounds of every plane at this depth"
        assert got.shape == want.shape == (n, v.frame_bytes(h, w, layout, bits))
        assert np.array_equal(got, want), ("egress", h, w, n, int((got != want).sum()))


def raw_calls(v):
    """The four entry points called as the library exports them, on contiguous tensors."""
    from ssm_amd import hipbind as hb
    from ssm_amd.frames import _f3, cfg_mean_std, padded_dims
    lib = hb.load()
    mean, std = (_f3(a) for a in cfg_mean_std(None))

    def ingest(x_entry, payload, h, w, matrix, crange, layout, sample_bytes=1, bits=8):
        (hp, wp), (top, left) = padded_dims(h, w)
        out = torch.full((payload.shape[0], 3, hp, wp), 7.0, device=DEV)
        args = (payload.data_ptr(), hb.view_of(out), payload.shape[0], h, w, hp, wp, top, left, mean, std, 1, v._table_ptr(bits), matrix, crange, layout)
        hb.check(lib.ssm_frames_from_yuvx_fwd(*args, sample_bytes, hb.stream_ptr()) if x_entry else lib.ssm_frames_from_yuv_fwd(*args, hb.stream_ptr()))
        return out

    def egress(x_entry, x, h, w, matrix, crange, layout, sample_bytes=1, bits=8):
        n, _, hp, wp = x.shape
        out = torch.full((n, v.frame_bytes(h, w, layout, bits)), 77, dtype=torch.uint8, device=DEV)
        args = (hb.view_of(x), out.data_ptr(), n, h, w, (hp - h) // 2, (wp - w) // 2, mean, std, v._table_ptr(bits), matrix, crange, layout)
        hb.check(lib.ssm_frames_to_yuvx_fwd(*args, sample_bytes, hb.stream_ptr()) if x_entry else lib.ssm_frames_to_yuv_fwd(*args, hb.stream_ptr()))
        return out

    return ingest, egress


@pytest.mark.parametrize("layout", [0, 1, 2])
def test_one_byte_samples_are_the_8_bit_entry_points(layout):
    v = V()
    ingest, egress = raw_calls(v)
    for (h, w), (matrix, crange) in itertools.product(SIZES, ((0, 0), (1, 1))):
        payload = torch.from_numpy(D.seeded_payload(3, h, w, layout, 8, 40 + layout)).to(DEV)
        a, b = ingest(False, payload, h, w, matrix, crange, layout), ingest(True, payload, h, w, matrix, crange, layout)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        x = torch.from_numpy(egress_input(np.random.RandomState(41 + layout), 3, h, w)).to(DEV)
        assert torch.equal(egress(False, x, h, w, matrix, crange, layout), egress(True, x, h, w, matrix, crange, layout))


def test_strided_views_on_both_sides_422p10():
    """Both kernels go through an ssm_view: a channel-offset, row-padded tensor gives the same planes and bytes as a contiguous one."""
    v = V()
    h, w, layout, bits = 46, 70, 3, 10
    payload = D.seeded_payload(2, h, w, layout, bits, 3)
    big = torch.full((2, 5, 66, 101), 7.0, device=DEV)
    out = big[:, 1:4, 1:65, 3:99]
    v.frames_from_yuv(torch.from_numpy(payload).to(DEV), h, w, layout, 1, 0, None, True, out=out, bits=bits)
    want = v.yuv_to_frames_host(payload, h, w, layout, 1, 0, bits=bits)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))
    rest = big.clone()
    rest[:, 1:4, 1:65, 3:99] = 7.0
    assert bool((rest == 7.0).all()), "the ingest kernel wrote outside its view"
    back = v.frames_to_yuv(out, h, w, layout, 1, 0, bits=bits).cpu().numpy()
    assert np.array_equal(back, v.frames_to_yuv_host(want, h, w, layout, 1, 0, bits=bits))


@pytest.mark.parametrize("layout,bits", [(0, 10), (3, 10), (2, 16), (3, 16)])
@pytest.mark.parametrize("h,w", [(64, 96), (46, 70)])
def test_scalar_paths_of_two_byte_samples(layout, bits, h, w):
    """A payload that starts 2 bytes into a buffer is 2-byte aligned and neither 4- nor 8-byte aligned: no wide store applies; likewise a
    width that is no multiple of 4.  The results are the yardstick's, and the bytes either side of the payload stay as they were."""
    v = V()
    n, fb = 2, v.frame_bytes(h, w, layout, bits)
    payload = D.seeded_payload(n, h, w, layout, bits, 50 + layout)
    buf = torch.full((n * fb + 16,), 77, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 8 == 0
    inner = buf[2:2 + n * fb].view(n, fb)
    inner.copy_(torch.from_numpy(payload))
    got = v.frames_from_yuv(inner, h, w, layout, 1, 0, bits=bits).cpu().numpy()
    want = v.yuv_to_frames_host(payload, h, w, layout, 1, 0, bits=bits)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    x = egress_input(np.random.RandomState(51), n, h, w)
    buf.fill_(77)
    v.frames_to_yuv(torch.from_numpy(x).to(DEV), h, w, layout, 1, 0, out=inner, bits=bits)
    host = buf.cpu().numpy()
    assert np.array_equal(host[2:2 + n * fb].reshape(n, fb), v.frames_to_yuv_host(x, h, w, layout, 1, 0, bits=bits))
    assert (host[:2] == 77).all() and (host[2 + n * fb:] == 77).all(), "the egress kernel wrote outside the payload"


def test_argument_errors_are_runtime_errors():
    from ssm_amd import hipbind as hb
    from ssm_amd.frames import _f3
    v = V()
    lib = hb.load()
    h, w = 8, 12
    payload = torch.zeros(1, v.frame_bytes(h, w, 3, 10) + 2, dtype=torch.uint8, device=DEV)
    before = payload.clone()
    x = torch.zeros(1, 3, 32, 32, device=DEV)
    mean, std, tab, st = _f3((0.5,) * 3), _f3((0.25,) * 3), v._table_ptr(10), hb.stream_ptr()

    def ingest(**kw):
        a = dict(p=payload.data_ptr(), out=hb.view_of(x), n=1, h=h, w=w, hp=32, wp=32, top=12, left=10, tab=tab, m=0, r=0, s=3, sb=2)
        a.update(kw)
        hb.check(lib.ssm_frames_from_yuvx_fwd(a["p"], a["out"], a["n"], a["h"], a["w"], a["hp"], a["wp"], a["top"], a["left"], mean, std, 1,
                                              a["tab"], a["m"], a["r"], a["s"], a["sb"], st))

    def egress(**kw):
        a = dict(p=payload.data_ptr(), inp=hb.view_of(x), n=1, h=h, w=w, top=12, left=10, tab=tab, m=0, r=0, s=3, sb=2)
        a.update(kw)
        hb.check(lib.ssm_frames_to_yuvx_fwd(a["inp"], a["p"], a["n"], a["h"], a["w"], a["top"], a["left"], mean, std, a["tab"], a["m"], a["r"],
                                            a["s"], a["sb"], st))

    ingest()
    egress()
    torch.cuda.synchronize()
    after_good = payload.clone()
    planes_good = x.clone()
    null = hb.SsmView(None, 0, 0, 0)
    for fn in (ingest, egress):
        for bad, pat in ((dict(p=payload.data_ptr() + 1), "2-byte aligned"), (dict(sb=0), "sample_bytes"), (dict(sb=3), "sample_bytes"),
                         (dict(s=4), "layout"), (dict(s=-1), "layout"), (dict(p=None), "null"), (dict(tab=None), "null"),
                         (dict(m=2), "matrix"), (dict(m=-1), "matrix"), (dict(r=2), "range"), (dict(n=0), "geometry"), (dict(h=0), "geometry"),
                         (dict(top=-1), "geometry"), (dict(w=40), "geometry")):
            with pytest.raises(RuntimeError, match=pat):
                fn(**bad)
    with pytest.raises(RuntimeError, match="null"):
        ingest(out=null)
    with pytest.raises(RuntimeError, match="null"):
        egress(inp=null)
    with pytest.raises(RuntimeError, match="geometry"):
        ingest(hp=16)
    torch.cuda.synchronize()
    assert torch.equal(payload, after_good) and torch.equal(x, planes_good), "a refused call launched nothing"
    assert not torch.equal(before, after_good), "the accepted egress call wrote the payload"
    ingest(p=payload.data_ptr() + 1, sb=1, s=0)          # one-byte samples may start anywhere
    torch.cuda.synchronize()


@pytest.mark.parametrize("bits", [10, 16])
@pytest.mark.parametrize("matrix,crange", [(0, 0), (1, 1), (1, 0), (0, 1)])
def test_in_gamut_round_trip_through_the_kernels_is_exact(bits, matrix, crange):
    v = V()
    colours, m = D.ingamut_pixels(200000, matrix, crange, bits, 900 + bits)
    x = v.frames_from_yuv(torch.from_numpy(colours).to(DEV), 1, m, v.C444, matrix, crange, bits=bits)
    back = v.frames_to_yuv(x, 1, m, v.C444, matrix, crange, bits=bits).cpu().numpy()
    assert m > 20000 and int((back.view("<u2") != colours.view("<u2")).sum()) == 0


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


def deep_clip(n, h, w, tag, seed=5):
    """A moving synthetic clip in the format of an extended tag, through the yardstick's egress: legal limited-range codes."""
    from ssm_amd.weights import IMAGENET_MEAN, IMAGENET_STD, synthetic_frames_u8
    v = V()
    layout, bits = v.EXTENDED_TAGS[tag]
    rgb = synthetic_frames_u8(n, h, w, seed=seed).numpy().astype(np.float32) / np.float32(255.0)
    x = (rgb - np.float32(IMAGENET_MEAN)[None, :, None, None]) / np.float32(IMAGENET_STD)[None, :, None, None]
    return v.frames_to_yuv_host(x, h, w, layout, v.default_matrix(h), v.LIMITED, bits=bits)


def clip_stream(payloads, h, w, tag, rate=(30, 1)):
    v = V()
    buf = io.BytesIO()
    with v.Y4MWriter(buf, w, h, rate=rate, aspect=(1, 1), chroma=tag, extended=True) as wr:
        for p in payloads:
            wr.write_frame(p)
    return io.BytesIO(buf.getvalue())


def read_deep(data):
    v = V()
    r = v.Y4MReader(io.BytesIO(data), extended=True)
    frames, buf = [], np.empty(r.frame_bytes, np.uint8)
    while r.read_frame_into(buf):
        frames.append(buf.copy())
    return r, np.stack(frames)


def run(m, cfg, payloads, h, w, tag, rate=(30, 1), out_rate=None, **kw):
    v = V()
    r = v.Y4MReader(clip_stream(payloads, h, w, tag, rate), extended=True)
    sink = io.BytesIO()
    wr = v.Y4MWriter.like(sink, r, rate=out_rate or r.rate)
    vi = v.VideoInterpolator(m, cfg, **kw)
    count = vi.run(r, wr)
    hdr, got = read_deep(sink.getvalue())
    assert got.shape[0] == count == wr.frames_written and hdr.chroma == tag
    return hdr, got, vi


@pytest.mark.parametrize("tag,streams", [("422", 2), ("420p10", 3), ("422p10", 2), ("444p16", 1)])
def test_streaming_equals_per_pair_evaluation(model, tag, streams):
    from ssm_amd.evaluation import t_values
    cfg, m = model
    v = V()
    h, w, n, rate = 64, 96, 10, 4
    layout, bits = v.EXTENDED_TAGS[tag]
    payloads = deep_clip(n, h, w, tag)
    hdr, got, _ = run(m, cfg, payloads, h, w, tag, out_rate=(30 * rate, 1), upsample_rate=rate, n_streams=streams, pairs_per_batch=1)
    assert got.shape[0] == (n - 1) * rate + 1 and hdr.rate == (30 * rate, 1) and (hdr.bits, hdr.siting) == (bits, layout)
    assert np.array_equal(got[::rate], payloads), "original frames must pass through as their own bytes"
    dev = torch.from_numpy(payloads).to(DEV)
    want = [payloads[0]]
    for i in range(n - 1):
        x = v.frames_from_yuv(dev[i:i + 2], h, w, layout, v.default_matrix(h), v.LIMITED, cfg, True, bits=bits)
        frames = m.interpolate(x[None], t_values(rate))
        want.extend(v.frames_to_yuv(frames, h, w, layout, v.default_matrix(h), v.LIMITED, cfg, bits=bits).cpu().numpy())
        want.append(payloads[i + 1])
    want = np.stack(want)
    assert np.array_equal(got, want), int((got != want).sum())


def test_target_rate_and_a_shutter_in_light_on_422p10(model):
    """60 -> 24 at 180 degrees in 4 samples, averaged in sRGB light: the stream against ingest -> FullModel.interpolate ->
    ssm_frames_accumulate_light_fwd sample by sample in time order -> egress."""
    from ssm_amd import hipbind as hb
    from ssm_amd.frames import cfg_mean_std
    cfg, m = model
    v = V()
    h, w, n, tag, S = 64, 96, 9, "422p10", 4
    layout, bits = v.EXTENDED_TAGS[tag]
    payloads = deep_clip(n, h, w, tag)
    hdr, got, _ = run(m, cfg, payloads, h, w, tag, rate=(60, 1), out_rate=(24, 1), n_streams=2, target_rate=(24, 1), shutter=Fr(1, 2),
                      shutter_samples=S, shutter_light="srgb")
    tl = v.Timeline(Fr(5, 2), shutter=Fr(1, 2), samples=S)
    assert got.shape[0] == tl.n_outputs(n) == 3 and hdr.rate == (24, 1)
    dev = torch.from_numpy(payloads).to(DEV)
    matrix, crange = v.default_matrix(h), v.LIMITED
    planes = v.frames_from_yuv(dev, h, w, layout, matrix, crange, cfg, True, bits=bits)
    made = {}
    for i in range(n - 1):
        ts = [float(v.Timeline.t32(t)) for t, _, _ in tl.times(i)]
        if ts:
            made[i] = m.interpolate(planes[i:i + 2][None], ts + [ts[-1]] * (tl.slots - len(ts)))
    mean, std = cfg_mean_std(cfg)
    row, scale, want = v.light_curve("srgb"), np.float32(1.0 / S), []
    for smp in tl.outputs(n):
        acc = torch.zeros((1,) + tuple(planes.shape[1:]), device=DEV)
        for j, (i, t) in enumerate(smp):
            frame = planes[i:i + 1] if t == 0 else made[i][[x for x, _, _ in tl.times(i)].index(t)][None]
            hb.frames_accumulate_light(frame.contiguous(), acc, 1 if j == 0 else 0, scale if j == S - 1 else 1.0, mean, std, row, 1 if j == S - 1 else 0)
        want.append(v.frames_to_yuv(acc, h, w, layout, matrix, crange, cfg, bits=bits).cpu().numpy()[0])
    want = np.stack(want)
    assert np.array_equal(got, want), int((got != want).sum())
    assert not np.array_equal(got[0], payloads[0]), "output 0 is a mean, not frame 0"


def test_scene_cuts_on_422_are_those_of_420jpeg(model):
    """The luma of a clip is the same bytes under both layouts, so the sums, the scores and the cut are."""
    import video_cut_clips as C
    cfg, m = model
    v = V()
    h, w = C.SIZES[0]
    found = {}
    for tag, layout in (("420jpeg", 0), ("422", 3)):
        from ssm_amd.weights import IMAGENET_MEAN, IMAGENET_STD, synthetic_frames_u8
        parts = []
        for count, seed in ((C.CUT + 1, 5), (C.N_FRAMES - C.CUT - 1, 6)):
            rgb = synthetic_frames_u8(count, h, w, seed=seed).numpy().astype(np.float32) / np.float32(255.0)
            x = (rgb - np.float32(IMAGENET_MEAN)[None, :, None, None]) / np.float32(IMAGENET_STD)[None, :, None, None]
            parts.append(v.frames_to_yuv_host(x, h, w, layout, v.default_matrix(h), v.LIMITED).copy())
        parts[0][:, :h * w] = 16 + (parts[0][:, :h * w] - 16) // 4
        parts[1][:, :h * w] = 235 - (parts[1][:, :h * w] - 16) // 4
        payloads = np.concatenate(parts)
        if layout == 0:
            assert np.array_equal(payloads, C.cut_clip(h, w))
        _, got, vi = run(m, cfg, payloads, h, w, tag, out_rate=(120, 1), upsample_rate=4, n_streams=2, scene_cut=C.THRESHOLD)
        found[tag] = (vi.cuts, payloads[:, :h * w])
        o = 4 * C.CUT
        assert np.array_equal(got[o + 1], payloads[C.CUT]) and np.array_equal(got[o + 2], payloads[C.CUT + 1])
    assert np.array_equal(found["422"][1], found["420jpeg"][1])
    assert found["422"][0] == found["420jpeg"][0] and [i for i, _ in found["422"][0]] == [C.CUT]


def test_scene_cuts_above_8_bits_are_refused_by_name(model):
    cfg, m = model
    payloads = deep_clip(3, 64, 96, "420p10")
    with pytest.raises(ValueError, match="scene_cut.*C420p10"):
        run(m, cfg, payloads, 64, 96, "420p10", upsample_rate=2, scene_cut=Fr(1, 10))


def test_cli_end_to_end_422p10(model, tmp_path):
    import interpolate_video
    cfg, m = model
    v = V()
    h, w, n, rate, tag = 40, 56, 3, 2, "422p10"
    payloads = deep_clip(n, h, w, tag)
    src, dst, ini = str(tmp_path / "in.y4m"), str(tmp_path / "out.y4m"), str(tmp_path / "cfg.ini")
    with open(src, "wb") as f:
        f.write(clip_stream(payloads, h, w, tag, rate=(60000, 1001)).getvalue())
    with open(ini, "w") as f:
        cfg.write(f)
    argv = ["-c", ini, "--expt", "t", "--log", str(tmp_path / "log.txt"), "--input", src, "--output", dst, "--upsample_rate", str(rate)]
    assert interpolate_video.main(argv, model=m) == (n - 1) * rate + 1
    with open(dst, "rb") as f:
        data = f.read()
    assert b" C422p10" in data.split(b"\n", 1)[0]
    hdr, got = read_deep(data)
    assert got.shape[0] == (n - 1) * rate + 1 and (hdr.width, hdr.height, hdr.chroma, hdr.bits) == (w, h, tag, 10)
    assert hdr.rate == (60000 * rate, 1001) and np.array_equal(got[::rate], payloads)
    with pytest.raises(v.Y4MError, match="C422p10"):
        read_clip(dst)          # a reader without the flag still refuses the tag
