"""Tiled inference on the GPU: ssm_tile_stitch_fwd against its numpy float32 yardstick (ssm_amd.tiles.stitch_host) - BIT-equal,
since kernel and yardstick perform the same rounded fp32 operations in the same order - and the TiledEngine, interpolate_many, the streamed
video loop and the command line against evaluations of the same kernels window by window.  The mode itself is an approximation of the
untiled output, not parity; nothing here compares it with untiled frames (tools/bench_tiled.py reports that distance)."""
import io

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
# (canvas, tile, halo): 2x2 tiles; 1x3 (a tile with a seam on both sides); 3x1 with a last core of 32 rows, shorter than a band of b = 32
GRIDS = (((128, 192), (64, 96), 32), ((64, 288), (64, 96), 32), ((160, 96), (64, 96), 32))
TS = (0.25, 0.5, 0.75)


def T():
    from ssm_amd import tiles
    return tiles


def H():
    from ssm_amd import hipbind
    return hipbind


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


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


def random_tiles(grid, N, C=3, seed=11):
    """Finite contents that differ from tile to tile (so the cross-fade mixes unequal values), signs and magnitudes mixed."""
    rng = np.random.RandomState(seed)
    return [(rng.standard_normal((N, C) + grid.window) * 10.0 ** rng.randint(-3, 4)).astype(np.float32) for _ in grid.tiles]


def stitch_all(grid, dev_tiles, out):
    hb = H()
    for tl, x in zip(grid.tiles, dev_tiles):
        hb.tile_stitch(x, out, (tl.y0, tl.x0), (tl.cy0, tl.cx0, tl.cy1, tl.cx1), tl.seams, grid.blend)
    torch.cuda.synchronize()
    return out


# ---- the kernel ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("b", [0, 8, 32])
@pytest.mark.parametrize("canvas,tile,halo", GRIDS)
def test_kernel_equals_the_yardstick_bit_for_bit(canvas, tile, halo, b, N):
    g = T().tile_grid(canvas, tile, halo, b)          # b = 0, 8 and 32 are legal on all three grids: none is dropped
    tiles = random_tiles(g, N)
    want = T().stitch_host(tiles, g)
    assert np.isfinite(want).all()
    out = torch.full((N, 3) + canvas, float("nan"), device=DEV)          # a pixel nobody wrote, or one read before its first store, shows
    got = stitch_all(g, [torch.from_numpy(x).to(DEV) for x in tiles], out).cpu().numpy()
    assert np.array_equal(bits(got), bits(want)), int((bits(got) != bits(want)).sum())


@pytest.mark.parametrize("xoff,rowpad", [(4, 8), (3, 7)])          # 16-byte aligned rows (the float4 kernel) and unaligned ones (one pixel per lane)
@pytest.mark.parametrize("canvas,tile,halo", GRIDS)
def test_strided_views_and_nothing_outside_them(canvas, tile, halo, xoff, rowpad):
    """Tiles and output as channel-offset, row-padded views of larger sentinel-filled tensors: same bits, sentinel intact around the view."""
    N, C, SENT = 2, 3, -12345.0
    g = T().tile_grid(canvas, tile, halo, 8)
    tiles = random_tiles(g, N, seed=12)
    want = T().stitch_host(tiles, g)
    wh, ww = g.window
    holders, views = [], []
    for x in tiles:
        big = torch.full((N, C + 2, wh + 3, ww + rowpad), SENT, device=DEV)
        v = big[:, 1:1 + C, 2:2 + wh, xoff:xoff + ww]
        v.copy_(torch.from_numpy(x))
        holders.append(big)
        views.append(v)
    big_out = torch.full((N, C + 3, canvas[0] + 5, canvas[1] + rowpad), SENT, device=DEV)
    out = big_out[:, 2:2 + C, 1:1 + canvas[0], xoff:xoff + canvas[1]]
    stitch_all(g, views, out)
    assert np.array_equal(bits(out.cpu().numpy()), bits(want))
    mask = torch.ones_like(big_out, dtype=torch.bool)
    mask[:, 2:2 + C, 1:1 + canvas[0], xoff:xoff + canvas[1]] = False
    assert bool((big_out[mask] == SENT).all()), "the stitch wrote outside the output view"
    for big, x in zip(holders, tiles):          # and the tiles are only read
        assert np.array_equal(bits(big[:, 1:1 + C, 2:2 + wh, xoff:xoff + ww].cpu().numpy()), bits(x))


def test_a_launch_writes_its_region_of_influence_only():
    g = T().tile_grid((128, 192), (64, 96), 32, 8)
    tl = g.tiles[3]
    out = torch.full((1, 3, 128, 192), float("nan"), device=DEV)
    H().tile_stitch(torch.ones((1, 3) + g.window, device=DEV), out, (tl.y0, tl.x0), (tl.cy0, tl.cx0, tl.cy1, tl.cx1), 0, 8)      # no seams: the core
    torch.cuda.synchronize()
    written = ~torch.isnan(out[0, 0]).cpu()
    want = torch.zeros(128, 192, dtype=torch.bool)
    want[tl.cy0:tl.cy1, tl.cx0:tl.cx1] = True
    assert torch.equal(written, want)


def test_argument_errors_are_runtime_errors():
    hb = H()
    lib = hb.load()
    x = torch.zeros(1, 3, 96, 128, device=DEV)
    y = torch.zeros(1, 3, 128, 192, device=DEV)
    vx, vy, st = hb.view_of(x), hb.view_of(y), hb.stream_ptr()

    def call(tile=vx, out=vy, wh=96, ww=128, Hp=128, Wp=192, oy=32, ox=64, core=(64, 96, 128, 192), seams=5, b=8):
        hb.check(lib.ssm_tile_stitch_fwd(tile, out, 1, 3, wh, ww, Hp, Wp, oy, ox, core[0], core[1], core[2], core[3], seams, b, st))

    call()
    with pytest.raises(RuntimeError, match="null"):
        call(tile=hb.NULL_VIEW)
    with pytest.raises(RuntimeError, match="null"):
        call(out=hb.NULL_VIEW)
    for kw in (dict(oy=64), dict(ox=96), dict(core=(64, 96, 160, 192)), dict(core=(64, 96, 128, 224)), dict(core=(64, 96, 64, 192)),
               dict(oy=-32), dict(core=(-32, 96, 128, 192))):
        with pytest.raises(RuntimeError, match="geometry.*outside the canvas"):
            call(**kw)
    with pytest.raises(RuntimeError, match="geometry.*smaller than the core"):
        call(oy=32, ox=64, core=(64, 64, 128, 192), seams=5, b=8)          # the core grown by b starts left of the window
    with pytest.raises(RuntimeError, match="geometry.*smaller than the core"):
        call(wh=64, oy=64, seams=5, b=8)          # a window of exactly the core has no room for the band
    with pytest.raises(RuntimeError, match="geometry.*seam on a canvas edge"):
        call(seams=10)          # bottom and right of the last tile
    with pytest.raises(RuntimeError, match="geometry.*between two seams"):
        call(Hp=256, core=(64, 96, 96, 192), seams=7, b=32, oy=32)
    for b in (3, 2, 12, -8, 2048):
        with pytest.raises(RuntimeError, match="blend"):
            call(b=b)
    torch.cuda.synchronize()


# ---- the engine ----------------------------------------------------------------------------------------------------------------------
def pair_for(canvas, frame=None, seed=7):
    from ssm_amd.weights import synthetic_frames
    h, w = frame or canvas
    x = synthetic_frames(2, h, w, seed=seed)          # [1,2,3,Hp,Wp], the frame centred in the canvas
    assert tuple(x.shape[-2:]) == tuple(canvas)
    return x.to(DEV)


def per_window_reference(m, pair, grid):
    """model.interpolate on each window's crop of the pair (the same kernels, the plan of the window's shape), stitched on the host."""
    wh, ww = grid.window
    img6 = pair.reshape(1, 6, *pair.shape[-2:])
    frames = [m.interpolate(img6[:, :, tl.y0:tl.y0 + wh, tl.x0:tl.x0 + ww].contiguous(), TS).cpu().numpy() for tl in grid.tiles]
    return T().stitch_host(frames, grid)


@pytest.mark.parametrize("canvas,tile,halo,frame,blend,mode", [
    (GRIDS[0][0], GRIDS[0][1], 32, (120, 180), 8, None),
    (GRIDS[0][0], GRIDS[0][1], 32, (120, 180), 8, "f32"),
    (GRIDS[1][0], GRIDS[1][1], 32, None, 8, None),
    (GRIDS[2][0], GRIDS[2][1], 32, None, 32, None)])
def test_engine_equals_per_window_evaluation(model, canvas, tile, halo, frame, blend, mode):
    _, m = model
    g = T().tile_grid(canvas, tile, halo, blend)
    pair = pair_for(canvas, frame)
    m.precision = mode
    try:
        want = per_window_reference(m, pair, g)
        got = m.interpolate(pair, TS, tile=tile, halo=halo, blend=blend).cpu().numpy()
    finally:
        m.precision = None
    assert got.shape == (3, 3) + canvas and np.isfinite(got).all()
    assert np.array_equal(bits(got), bits(want)), float(np.abs(got - want).max())


def test_a_tile_that_covers_the_canvas_is_the_untiled_call(model):
    _, m = model
    pair = pair_for((128, 192), (120, 180))
    plain = m.interpolate(pair, TS).cpu().numpy()
    for tile in ((128, 192), (256, 192)):
        assert np.array_equal(bits(m.interpolate(pair, TS, tile=tile, halo=32, blend=8).cpu().numpy()), bits(plain))


def test_interpolate_many_equals_per_pair_calls(model):
    _, m = model
    pairs = [pair_for((128, 192), (120, 180), seed=s) for s in (3, 4, 5)]
    kw = dict(tile=(64, 96), halo=32, blend=8)
    many = m.interpolate_many(pairs, TS, n_streams=2, pairs_per_batch=1, **kw)
    assert len(many) == 3
    for pr, got in zip(pairs, many):
        assert np.array_equal(bits(got.cpu().numpy()), bits(m.interpolate(pr, TS, **kw).cpu().numpy()))


def test_refusals(model):
    from ssm_amd.config import load_config, synthetic_weight_overrides
    from ssm_amd.engine import PairPipeline
    from models.superslomo_r import FullModel
    _, m = model
    pair = pair_for((128, 192), (120, 180))
    with pytest.raises(NotImplementedError, match="tile=64x96 together with flow_scale=2"):
        m.interpolate(pair, TS, flow_scale=2, tile=(64, 96), halo=32)
    with pytest.raises(NotImplementedError, match="tile=64x96 together with flow_scale=2"):
        m.interpolate_many([pair], TS, flow_scale=2, tile=(64, 96), halo=32)
    rec = FullModel(load_config("superslomo_recurrent.ini", synthetic_weight_overrides()))
    with pytest.raises(NotImplementedError, match="tile=64x96 is not available with a recurrent bottleneck"):
        rec.interpolate(pair, TS, tile=(64, 96), halo=32)
    with pytest.raises(NotImplementedError, match=r"graphs=True\) does not cover tile=64x96"):
        PairPipeline({}, {}, 3, 128, 192, DEV, graphs=True, tile=(64, 96), halo=32)
    eng = m.tiled_engine_for(1, 3, 128, 192, DEV, (64, 96), 32, 8)
    with pytest.raises(NotImplementedError, match="flows of different tiles are not one field"):
        eng.intermediates()


def test_tiled_engine_allocates_less_than_the_plain_engine_of_the_canvas(model):
    """A condition, not a measurement: activations scale with the area and the 160 x 224 windows have 0.36 of the 256 x 384 canvas's."""
    from ssm_amd.engine import PairEngine, TiledEngine
    _, m = model
    m._drop_plans()
    sd1 = {k: v.detach() for k, v in m.stage1_model.state_dict().items()}
    sd2 = {k: v.detach() for k, v in m.stage2_model.state_dict().items()}
    H_, W_, nt = 256, 384, 3

    def growth(build):
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated(DEV)
        eng = build()
        torch.cuda.synchronize()
        grown = torch.cuda.memory_allocated(DEV) - before
        del eng
        return grown

    tiled = growth(lambda: TiledEngine(sd1, sd2, 1, nt, H_, W_, DEV, (128, 192), 32, 32, m.cross_skip, "f32w"))
    plain = growth(lambda: PairEngine(sd1, sd2, 1, nt, H_, W_, DEV, m.cross_skip, "f32w"))
    print("device memory of the engine at 256x384, 3 times: tiled (128x192 + 32) %d B, plain %d B" % (tiled, plain))
    assert 0 < tiled < plain, (tiled, plain)


# ---- the video path ------------------------------------------------------------------------------------------------------------------
def clip_payloads(n, h, w, siting=0, seed=5):
    """A moving synthetic clip as Y4M payloads [n, frame_bytes] uint8 (through the yardstick's egress: legal limited-range codes)."""
    from ssm_amd import video as v
    from ssm_amd.weights import synthetic_frames_u8, IMAGENET_MEAN, IMAGENET_STD
    rgb = synthetic_frames_u8(n, h, w, seed=seed).numpy().astype(np.float32) / np.float32(255.0)
    x = (rgb - np.float32(IMAGENET_MEAN)[None, :, None, None]) / np.float32(IMAGENET_STD)[None, :, None, None]
    return v.frames_to_yuv_host(x, h, w, siting, v.default_matrix(h), v.LIMITED)


def clip_file(payloads, h, w):
    from ssm_amd import video as v
    buf = io.BytesIO()
    with v.Y4MWriter(buf, w, h, rate=(30, 1), aspect=(1, 1), chroma="420jpeg") as wr:
        for p in payloads:
            wr.write_frame(p)
    buf.seek(0)
    return buf


def read_clip(src):
    from ssm_amd import video as v
    with v.Y4MReader(src) as r:
        frames, buf = [], np.empty(r.frame_bytes, np.uint8)
        while r.read_frame_into(buf):
            frames.append(buf.copy())
        return np.stack(frames)


def run_video(m, cfg, payloads, h, w, rate, **kw):
    from ssm_amd import video as v
    r = v.Y4MReader(clip_file(payloads, h, w))
    sink = io.BytesIO()
    wr = v.Y4MWriter.like(sink, r)
    count = v.VideoInterpolator(m, cfg, upsample_rate=rate, **kw).run(r, wr)
    assert count == wr.frames_written
    return read_clip(io.BytesIO(sink.getvalue()))


def per_pair_reference(m, cfg, payloads, h, w, rate, **tiling):
    """ingest -> tiled FullModel.interpolate -> egress of each pair on its own, originals in between: the expected output stream."""
    from ssm_amd import video as v
    from ssm_amd.evaluation import t_values
    dev = torch.from_numpy(payloads).to(DEV)
    out = [payloads[0]]
    for i in range(len(payloads) - 1):
        x = v.frames_from_yuv(dev[i:i + 2], h, w, 0, v.default_matrix(h), v.LIMITED, cfg, True)
        frames = m.interpolate(x[None], t_values(rate), **tiling)
        out.extend(v.frames_to_yuv(frames, h, w, 0, v.default_matrix(h), v.LIMITED, cfg).cpu().numpy())
        out.append(payloads[i + 1])
    return np.stack(out)


TILING = dict(tile=(64, 96), halo=32, blend=8)


@pytest.fixture(scope="module")
def clip_one_pair_per_pass(model):
    """The 10-frame 64x288 clip and its tiled output at one pair per pass: computed once, read by both video tests."""
    cfg, m = model
    h, w, n, rate = 64, 288, 10, 4
    payloads = clip_payloads(n, h, w)
    return payloads, run_video(m, cfg, payloads, h, w, rate, n_streams=2, pairs_per_batch=1, **TILING)


def test_video_one_pair_per_pass_equals_per_pair_evaluation(model, clip_one_pair_per_pass):
    cfg, m = model
    h, w, n, rate = 64, 288, 10, 4
    payloads, got = clip_one_pair_per_pass
    assert got.shape[0] == (n - 1) * rate + 1
    assert np.array_equal(got[::rate], payloads), "original frames must pass through as their own bytes"
    want = per_pair_reference(m, cfg, payloads, h, w, rate, **TILING)
    assert np.array_equal(got, want), int((got != want).sum())


def test_video_two_pairs_per_pass_keeps_count_and_originals(model, clip_one_pair_per_pass):
    cfg, m = model
    h, w, n, rate = 64, 288, 10, 4
    payloads, ref = clip_one_pair_per_pass
    got = run_video(m, cfg, payloads, h, w, rate, n_streams=2, pairs_per_batch=2, **TILING)
    assert got.shape[0] == (n - 1) * rate + 1 and np.array_equal(got[::rate], payloads)
    # the bound of tests/test_hip_video.py test_batched_passes_keep_count_order_and_originals, for its reason: a two-pair pass runs its
    # convolutions at batch 2, where the plan may pick other tiles; fp32 sums in another order can flip a code only at a tie - by one
    assert np.abs(got.astype(int) - ref.astype(int)).max() <= 1


def test_cli_end_to_end(model, tmp_path):
    import interpolate_video
    from ssm_amd import video as v
    cfg, m = model
    h, w, n, rate = 64, 192, 3, 2
    payloads = clip_payloads(n, h, w)
    src, dst, ini = str(tmp_path / "in.y4m"), str(tmp_path / "out.y4m"), str(tmp_path / "cfg.ini")
    with open(src, "wb") as f:
        f.write(clip_file(payloads, h, w).getvalue())
    with open(ini, "w") as f:
        cfg.write(f)
    argv = ["-c", ini, "--expt", "t", "--log", str(tmp_path / "log.txt"), "--input", src, "--output", dst, "--upsample_rate", str(rate),
            "--tile", "64x96", "--halo", "32", "--blend", "8"]
    assert interpolate_video.main(argv, model=m) == (n - 1) * rate + 1
    got = read_clip(dst)
    want = run_video(m, cfg, payloads, h, w, rate, **TILING)
    assert got.shape[0] == (n - 1) * rate + 1 and np.array_equal(got, want)
    untiled = run_video(m, cfg, payloads, h, w, rate)
    assert not np.array_equal(got, untiled), "the flags must reach the engine: tiled frames are not the untiled ones"
