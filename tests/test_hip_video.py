"""The video path on the GPU: the two kernels of csrc/ssm_video.hip against their numpy float32 yardsticks (ssm_amd.video.
yuv_to_frames_host / frames_to_yuv_host, themselves held to a float64 evaluation in tests/test_video_cpu.py) - BIT-equal planes and
BYTE-equal codes, since kernel and yardstick perform the same rounded fp32 operations in the same order on the same fp32 constants -
and the streamed loop (VideoInterpolator, scripts/interpolate_video.py) against a pair-by-pair evaluation of the same kernels."""
import io
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from video_clips import V, clip_payloads, read_clip, write_clip  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SIZES = ((46, 70), (45, 71), (64, 96))          # even, odd (offsets 9/13 and 9/12 in the 64 x 96 canvas), and a canvas-filling size


def make_model():
    from models.superslomo_r import FullModel
    from ssm_amd.config import load_config, synthetic_weight_overrides
    from ssm_amd.weights import synthetic_state_dict
    cfg = load_config("superslomo_original.ini", synthetic_weight_overrides())
    m = FullModel(cfg)
    m.stage1_model.load_state_dict(synthetic_state_dict(1))
    m.stage2_model.load_state_dict(synthetic_state_dict(2))
    return cfg, m.to(DEV).eval()


@pytest.fixture(scope="module")
def model():
    return make_model()


@pytest.mark.parametrize("siting,matrix,crange", list(itertools.product((0, 1, 2), (0, 1), (0, 1))))
def test_kernels_equal_their_yardsticks(siting, matrix, crange):
    v = V()
    for (h, w), n, pbn in itertools.product(SIZES, (1, 3), (True, False)):
        rng = np.random.RandomState(1000 * siting + 100 * matrix + 10 * crange + n)
        payload = rng.randint(0, 256, size=(n, v.frame_bytes(h, w, siting))).astype(np.uint8)
        got = v.frames_from_yuv(torch.from_numpy(payload).to(DEV), h, w, siting, matrix, crange, None, pbn).cpu().numpy()
        want = v.yuv_to_frames_host(payload, h, w, siting, matrix, crange, pad_before_norm=pbn)
        assert got.shape == want.shape
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), \
            ("ingest", h, w, n, pbn, float(np.abs(got - want).max()), int((got != want).sum()))
    for (h, w), n in itertools.product(SIZES, (1, 3)):
        rng = np.random.RandomState(7 + 1000 * siting + 100 * matrix + 10 * crange + n)
        hp, wp = -(-h // 32) * 32, -(-w // 32) * 32
        x = rng.uniform(-4.5, 5.0, size=(n, 3, hp, wp)).astype(np.float32)          # denormalised about -0.55 .. 1.55
        for i, rgb in enumerate(((-4.5, -4.5, 5.0), (5.0, 5.0, -4.5), (5.0, -4.5, -4.5), (-4.5, 5.0, 5.0), (5.0, 5.0, 5.0), (-4.5, -4.5, -4.5))):
            x[:, :, hp // 2 - 2:hp // 2 + 2, wp // 2 - 12 + 4 * i:wp // 2 - 8 + 4 * i] = np.float32(rgb)[None, :, None, None]          # both bounds of every plane
        got = v.frames_to_yuv(torch.from_numpy(x).to(DEV), h, w, siting, matrix, crange).cpu().numpy()
        want = v.frames_to_yuv_host(x, h, w, siting, matrix, crange)
        lo, hi, chi = (16, 235, 240) if crange == v.LIMITED else (0, 255, 255)
        assert want[:, :h * w].min() == lo and want[:, :h * w].max() == hi and want[:, h * w:].min() == lo and want[:, h * w:].max() == chi
        assert np.array_equal(got, want), ("egress", h, w, n, int((got != want).sum()), int(np.abs(got.astype(int) - want.astype(int)).max()))


def test_egress_reads_strided_views_and_ingest_writes_them():
    """Both kernels go through an ssm_view: a channel-offset, row-padded tensor gives the same bytes as a contiguous one."""
    v = V()
    h, w = 46, 70
    rng = np.random.RandomState(3)
    payload = rng.randint(0, 256, size=(2, v.frame_bytes(h, w, 0))).astype(np.uint8)
    big = torch.full((2, 5, 66, 101), 7.0, device=DEV)
    out = big[:, 1:4, 1:65, 3:99]
    v.frames_from_yuv(torch.from_numpy(payload).to(DEV), h, w, 0, 1, 0, None, True, out=out)
    want = v.yuv_to_frames_host(payload, h, w, 0, 1, 0)
    assert np.array_equal(out.cpu().numpy(), want)
    rest = big.clone()
    rest[:, 1:4, 1:65, 3:99] = 7.0
    assert bool((rest == 7.0).all()), "the ingest kernel wrote outside its view"
    back = v.frames_to_yuv(out, h, w, 0, 1, 0).cpu().numpy()
    assert np.array_equal(back, v.frames_to_yuv_host(want, h, w, 0, 1, 0))


@pytest.mark.parametrize("pbn", [False, True])
def test_pad_ring_is_the_rgb_kernels(pbn):
    from ssm_amd import frames as F
    v = V()
    h, w = 45, 71
    rng = np.random.RandomState(11)
    payload = torch.from_numpy(rng.randint(0, 256, size=(2, v.frame_bytes(h, w, 0))).astype(np.uint8)).to(DEV)
    got = v.frames_from_yuv(payload, h, w, 0, 0, 0, None, pbn)
    ref = F.frames_from_u8(torch.zeros(2, h, w, 3, dtype=torch.uint8, device=DEV), None, pad_before_norm=pbn)
    (hp, wp), (top, left) = F.padded_dims(h, w)
    ring = torch.ones(hp, wp, dtype=torch.bool, device=DEV)
    ring[top:top + h, left:left + w] = False
    assert got.shape == ref.shape and torch.equal(got[:, :, ring], ref[:, :, ring])
    assert (not pbn and float(got[:, :, ring].abs().max()) == 0.0) or (pbn and float(got[:, :, ring].abs().min()) > 1.0)


def test_argument_errors_are_runtime_errors():
    from ssm_amd import hipbind as hb
    from ssm_amd.frames import _f3
    v = V()
    lib = hb.load()
    h, w = 8, 12
    payload = torch.zeros(1, v.frame_bytes(h, w, 0), dtype=torch.uint8, device=DEV)
    x = torch.zeros(1, 3, 32, 32, device=DEV)
    mean, std, tab, st = _f3((0.5,) * 3), _f3((0.25,) * 3), v._table_ptr(), hb.stream_ptr()

    def ingest(**kw):
        a = dict(p=payload.data_ptr(), out=hb.view_of(x), n=1, h=h, w=w, hp=32, wp=32, top=12, left=10, tab=tab, m=0, r=0, s=0)
        a.update(kw)
        hb.check(lib.ssm_frames_from_yuv_fwd(a["p"], a["out"], a["n"], a["h"], a["w"], a["hp"], a["wp"], a["top"], a["left"], mean, std, 1,
                                             a["tab"], a["m"], a["r"], a["s"], st))

    def egress(**kw):
        a = dict(p=payload.data_ptr(), inp=hb.view_of(x), n=1, h=h, w=w, top=12, left=10, tab=tab, m=0, r=0, s=0)
        a.update(kw)
        hb.check(lib.ssm_frames_to_yuv_fwd(a["inp"], a["p"], a["n"], a["h"], a["w"], a["top"], a["left"], mean, std, a["tab"], a["m"], a["r"],
                                           a["s"], st))

    ingest()
    egress()
    null = hb.SsmView(None, 0, 0, 0)
    for fn in (ingest, egress):
        for bad, pat in ((dict(p=None), "null"), (dict(tab=None), "null"), (dict(m=2), "matrix"), (dict(m=-1), "matrix"), (dict(r=2), "range"),
                         (dict(s=3), "siting"), (dict(s=-1), "siting"), (dict(n=0), "geometry"), (dict(h=0), "geometry"),
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


def per_pair_reference(model, cfg, payloads, h, w, siting, matrix, crange, rate):
    """ingest -> FullModel.interpolate -> egress of each pair on its own, originals in between: the expected output stream."""
    from ssm_amd.evaluation import t_values
    v = V()
    dev = torch.from_numpy(payloads).to(DEV)
    out = [payloads[0]]
    for i in range(len(payloads) - 1):
        x = v.frames_from_yuv(dev[i:i + 2], h, w, siting, matrix, crange, cfg, True)
        frames = model.interpolate(x[None], t_values(rate))
        out.extend(v.frames_to_yuv(frames, h, w, siting, matrix, crange, cfg).cpu().numpy())
        out.append(payloads[i + 1])
    return np.stack(out)


@pytest.mark.parametrize("chroma,pb,streams", [("420jpeg", 1, 2), ("420mpeg2", 1, 3), ("444", 1, 1)])
def test_streaming_equals_per_pair_evaluation(model, tmp_path, chroma, pb, streams):
    cfg, m = model
    v = V()
    h, w, n, rate = 64, 96, 10, 4
    siting = v.CHROMA_TAGS[chroma]
    payloads = clip_payloads(n, h, w, siting)
    src, dst = str(tmp_path / "in.y4m"), str(tmp_path / "out.y4m")
    write_clip(src, payloads, h, w, chroma)
    vi = v.VideoInterpolator(m, cfg, upsample_rate=rate, n_streams=streams, pairs_per_batch=pb)
    with v.Y4MReader(src) as r, v.Y4MWriter.like(dst, r, rate=v.output_rate(r.rate, rate)) as wr:
        count = vi.run(r, wr)
    assert count == (n - 1) * rate + 1
    hdr, got = read_clip(dst)
    assert got.shape[0] == count and hdr.chroma == chroma and hdr.rate == (30 * rate, 1)
    assert np.array_equal(got[::rate], payloads), "original frames must pass through as their own bytes"
    want = per_pair_reference(m, cfg, payloads, h, w, siting, v.default_matrix(h), v.LIMITED, rate)
    assert np.array_equal(got, want), int((got != want).sum())


def test_batched_passes_keep_count_order_and_originals(model, tmp_path):
    """pairs_per_batch = 2 over an odd number of pairs: the last pass is filled and its extra pair not written."""
    cfg, m = model
    v = V()
    h, w, n, rate = 64, 96, 6, 2
    payloads = clip_payloads(n, h, w, 0)
    buf_in = io.BytesIO()
    write_clip(buf_in, payloads, h, w)
    buf_in.seek(0)
    buf_out = io.BytesIO()
    r = v.Y4MReader(buf_in)
    wr = v.Y4MWriter.like(buf_out, r)
    count = v.VideoInterpolator(m, cfg, upsample_rate=rate, n_streams=2, pairs_per_batch=2).run(r, wr)
    assert count == (n - 1) * rate + 1 == wr.frames_written
    _, got = read_clip(io.BytesIO(buf_out.getvalue()))
    assert got.shape[0] == count and np.array_equal(got[::rate], payloads)
    one = io.BytesIO()
    buf_in.seek(0)
    r1 = v.Y4MReader(buf_in)
    v.VideoInterpolator(m, cfg, upsample_rate=rate, n_streams=1, pairs_per_batch=1).run(r1, v.Y4MWriter.like(one, r1))
    _, ref = read_clip(io.BytesIO(one.getvalue()))
    # a two-pair pass runs its convolutions at batch 2, where the plan may pick other tiles: fp32 sums in another order move a frame by
    # ~1e-5 of full scale (the precision modes sit 2e-4 from the oracle at most: 0.05 code), so a code can only flip at a tie - by one
    assert np.abs(got.astype(int) - ref.astype(int)).max() <= 1


def test_device_memory_is_flat_in_clip_length(model, tmp_path):
    cfg, m = model
    v = V()
    h, w, rate = 64, 96, 4
    vi = v.VideoInterpolator(m, cfg, upsample_rate=rate, n_streams=2, pairs_per_batch=1)
    peaks = []
    for n in (8, 8, 40):          # the first run also builds the plans
        payloads = clip_payloads(n, h, w, 0)
        buf_in = io.BytesIO()
        write_clip(buf_in, payloads, h, w)
        buf_in.seek(0)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(DEV)
        r = v.Y4MReader(buf_in)
        sink = open(os.devnull, "wb")
        assert vi.run(r, v.Y4MWriter.like(sink, r)) == (n - 1) * rate + 1
        sink.close()
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated(DEV))
    print("peak device memory: 8 frames %d B, 40 frames %d B" % (peaks[1], peaks[2]))
    assert peaks[2] <= peaks[1], peaks


def test_n_frames_other_than_two_is_refused(model):
    import copy
    cfg, m = model
    v = V()
    cfg4 = copy.deepcopy(cfg)
    cfg4.set("TRAIN", "N_FRAMES", "4")
    with pytest.raises(NotImplementedError, match="N_FRAMES=4"):
        v.VideoInterpolator(m, cfg4)


@pytest.mark.parametrize("slowmo", [False, True])
def test_cli_end_to_end(model, tmp_path, slowmo):
    import interpolate_video
    from ssm_amd.config import synthetic_weight_overrides
    cfg, m = model
    v = V()
    h, w, n, rate = 40, 56, 3, 2
    payloads = clip_payloads(n, h, w, 0)
    src, dst, ini = str(tmp_path / "in.y4m"), str(tmp_path / "out.y4m"), str(tmp_path / "cfg.ini")
    write_clip(src, payloads, h, w, rate=(30000, 1001), color_range=v.FULL)
    with open(ini, "w") as f:
        cfg.write(f)
    argv = ["-c", ini, "--expt", "t", "--log", str(tmp_path / "log.txt"), "--input", src, "--output", dst, "--upsample_rate", str(rate),
            "--matrix", "bt709"] + (["--slowmo"] if slowmo else [])
    assert interpolate_video.main(argv, model=m) == (n - 1) * rate + 1
    hdr, got = read_clip(dst)
    assert got.shape[0] == (n - 1) * rate + 1 and (hdr.width, hdr.height, hdr.chroma) == (w, h, "420jpeg")
    assert hdr.rate == ((30000, 1001) if slowmo else (30000 * rate, 1001))
    assert hdr.color_range == v.FULL, "the input's XCOLORRANGE tag is honoured and written"
    assert np.array_equal(got[::rate], payloads)
    want = per_pair_reference(m, cfg, payloads, h, w, 0, v.BT709, v.FULL, rate)
    assert np.array_equal(got, want)
