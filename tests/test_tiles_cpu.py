"""Tiled inference without a GPU (ssm_amd/tiles.py): grids worked by hand, the cross-fade weights (exact in float32: they sum
to exactly 1 over every canvas pixel and every pixel has one first tile), the numpy yardstick of the stitch on integer-valued images,
every argument error by name, and the flags of the two command lines."""
import numpy as np
import pytest

# (canvas, tile, halo) of the three hand-worked grids and of a tile that covers its canvas
GRIDS = (((128, 192), (64, 96), 32), ((64, 288), (64, 96), 32), ((160, 96), (64, 96), 32))
BLENDS = (0, 4, 8, 32)


def T():
    from ssm_amd import tiles
    return tiles


def test_module_is_host_only():
    import re
    src = open(T().__file__).read()
    assert not re.search(r"^\s*(from|import)\s+(torch|oracle|ssm_oracle)\b", src, re.M), "tiles.py is pure Python / numpy"


def test_grid_2x2():
    t = T()
    g = t.tile_grid((128, 192), (64, 96), halo=32, blend=8)
    assert (g.ny, g.nx, len(g)) == (2, 2, 4) and g.window == (96, 128)
    assert [(tl.y0, tl.x0) for tl in g.tiles] == [(0, 0), (0, 64), (32, 0), (32, 64)]
    assert [(tl.cy0, tl.cy1, tl.cx0, tl.cx1) for tl in g.tiles] == [(0, 64, 0, 96), (0, 64, 96, 192), (64, 128, 0, 96), (64, 128, 96, 192)]
    assert [tl.seams for tl in g.tiles] == [t.SEAM_BOTTOM | t.SEAM_RIGHT, t.SEAM_BOTTOM | t.SEAM_LEFT, t.SEAM_TOP | t.SEAM_RIGHT,
                                            t.SEAM_TOP | t.SEAM_LEFT]
    assert g.region(g.tiles[0]) == (0, 72, 0, 104) and g.region(g.tiles[3]) == (56, 128, 88, 192)


def test_grid_1x3():
    t = T()
    g = t.tile_grid((64, 288), (64, 96), halo=32, blend=8)
    assert (g.ny, g.nx) == (1, 3) and g.window == (64, 160)
    assert [tl.x0 for tl in g.tiles] == [0, 64, 128] and all(tl.y0 == 0 for tl in g.tiles)
    assert [(tl.cx0, tl.cx1) for tl in g.tiles] == [(0, 96), (96, 192), (192, 288)]
    assert [tl.seams for tl in g.tiles] == [t.SEAM_RIGHT, t.SEAM_LEFT | t.SEAM_RIGHT, t.SEAM_LEFT]


def test_grid_3x1_with_a_short_last_core():
    t = T()
    g = t.tile_grid((160, 96), (64, 96), halo=32, blend=32)
    assert (g.ny, g.nx) == (3, 1) and g.window == (128, 96)
    assert [(tl.cy0, tl.cy1) for tl in g.tiles] == [(0, 64), (64, 128), (128, 160)]
    assert [tl.y0 for tl in g.tiles] == [0, 32, 32] and all(tl.x0 == 0 for tl in g.tiles)
    assert g.region(g.tiles[1]) == (32, 160, 0, 96), "the band behind the short last core is cut at the canvas"


def test_tile_that_covers_the_canvas():
    t = T()
    for tile in ((128, 192), (160, 256)):
        g = t.tile_grid((128, 192), tile, halo=32, blend=8)
        assert len(g) == 1 and g.window == (128, 192) and t.covers_canvas((128, 192), tile)
        tl = g.tiles[0]
        assert (tl.y0, tl.x0, tl.cy0, tl.cy1, tl.cx0, tl.cx1, tl.seams) == (0, 0, 0, 128, 0, 192, 0)
    assert not t.covers_canvas((128, 192), (128, 96))


def test_every_window_holds_its_region_and_origins_are_multiples_of_32():
    t = T()
    for canvas in ((128, 192), (160, 96), (2176, 3840), (4320, 7680), (736, 1280)):
        for tile, halo, b in (((64, 96), 32, 32), ((64, 64), 256, 32), ((1088, 1920), 256, 32), ((2176, 3840), 256, 256), ((352, 640), 64, 0)):
            g = t.tile_grid(canvas, tile, halo, b)
            cover = np.zeros(canvas, int)
            for tl in g.tiles:
                ry0, ry1, rx0, rx1 = g.region(tl)
                assert tl.y0 % 32 == 0 and tl.x0 % 32 == 0 and g.window[0] % 32 == 0 and g.window[1] % 32 == 0
                assert 0 <= tl.y0 <= ry0 < ry1 <= tl.y0 + g.window[0] <= canvas[0]
                assert 0 <= tl.x0 <= rx0 < rx1 <= tl.x0 + g.window[1] <= canvas[1]
                cover[tl.cy0:tl.cy1, tl.cx0:tl.cx1] += 1
            assert (cover == 1).all(), "the cores partition the canvas"


def legal(tile, halo, b):
    return b <= halo and 2 * b <= min(tile)


@pytest.mark.parametrize("b", BLENDS)
@pytest.mark.parametrize("canvas,tile,halo", GRIDS)
def test_weights_sum_to_exactly_one_and_every_pixel_has_one_first_tile(canvas, tile, halo, b):
    t = T()
    assert legal(tile, halo, b)          # all four are legal on these grids: none is dropped
    g = t.tile_grid(canvas, tile, halo, b)
    total = np.zeros(canvas, np.float32)
    firsts = np.zeros(canvas, int)
    for tl in g.tiles:          # raster order, the kernel's accumulation order
        ry0, ry1, rx0, rx1 = g.region(tl)
        w, first = t.tile_weights(g, tl)
        assert w.dtype == np.float32 and w.shape == first.shape == (ry1 - ry0, rx1 - rx0)
        assert (w > 0).all() and (w <= 1).all()
        exact = w.astype(np.float64) * float(max(4 * b, 1)) ** 2          # dyadic with few bits
        assert (exact == np.rint(exact)).all()
        total[ry0:ry1, rx0:rx1] = total[ry0:ry1, rx0:rx1] + w
        firsts[ry0:ry1, rx0:rx1] += first
    assert (total == np.float32(1.0)).all(), float(np.abs(total - 1).max())
    assert (firsts == 1).all()


@pytest.mark.parametrize("b", BLENDS)
@pytest.mark.parametrize("canvas,tile,halo", GRIDS + (((128, 192), (128, 192), 32),))
def test_stitch_host_returns_an_integer_image_bit_for_bit(canvas, tile, halo, b):
    t = T()
    g = t.tile_grid(canvas, tile, halo, b)
    rng = np.random.RandomState(3)
    img = rng.randint(-4096, 4096, size=(2, 3) + canvas).astype(np.float32)
    wh, ww = g.window
    cuts = [img[:, :, tl.y0:tl.y0 + wh, tl.x0:tl.x0 + ww] for tl in g.tiles]
    out = t.stitch_host(cuts, g)
    assert out.dtype == np.float32 and np.array_equal(out.view(np.uint32), img.view(np.uint32))
    # ... and into a caller's array, which the first store of every pixel overwrites whatever it held
    into = np.full_like(img, np.nan)
    assert t.stitch_host(cuts, g, out=into) is into and np.array_equal(into.view(np.uint32), img.view(np.uint32))


def test_stitch_host_cross_fades_tiles_that_differ():
    """Two constant tiles, 1 and 3, side by side: the seam is the ramp 1 + 2 u(x), every value exact."""
    t = T()
    g = t.tile_grid((64, 192), (64, 96), halo=32, blend=4)
    tiles = [np.full((1, 1) + g.window, v, np.float32) for v in (1.0, 3.0)]
    row = t.stitch_host(tiles, g)[0, 0, 17]
    assert (row[:92] == 1).all() and (row[100:] == 3).all()
    assert np.array_equal(row[92:100], 1 + 2 * (np.arange(8) + 0.5) / 8)


def test_argument_errors_name_their_value():
    t = T()
    for bad, msg in ((dict(tile=(65, 96)), "tile height must be a multiple of 32 and at least 64 \\(got 65\\)"),
                     (dict(tile=(64, 100)), "tile width must be a multiple of 32 and at least 64 \\(got 100\\)"),
                     (dict(tile=(32, 96)), "tile height must be a multiple of 32 and at least 64 \\(got 32\\)"),
                     (dict(tile=1088), "tile must be a pair \\(th, tw\\) of core sizes \\(got 1088\\)"),
                     (dict(halo=0), "halo must be a multiple of 32 and at least 32 \\(got 0\\)"),
                     (dict(halo=16), "halo must be a multiple of 32 and at least 32 \\(got 16\\)"),
                     (dict(halo=48), "halo must be a multiple of 32 and at least 32 \\(got 48\\)"),
                     (dict(blend=3), "blend must be 0 or a power of two >= 4 \\(got 3\\)"),
                     (dict(blend=2), "blend must be 0 or a power of two >= 4 \\(got 2\\)"),
                     (dict(blend=12), "blend must be 0 or a power of two >= 4 \\(got 12\\)"),
                     (dict(blend=-4), "blend must be 0 or a power of two >= 4 \\(got -4\\)"),
                     (dict(blend=64, halo=32), "blend must not exceed the halo \\(got blend 64 > halo 32\\)"),
                     (dict(blend=64, halo=64), "2 \\* blend <= tile size \\(got blend 64, tile 64x96\\)"),
                     (dict(blend=2048, halo=2048, tile=(4096, 4096)), "blend must not exceed 1024")):
        kw = dict(tile=(64, 96), halo=32, blend=8)
        kw.update(bad)
        with pytest.raises(ValueError, match=msg):
            t.check_args(**kw)
        with pytest.raises(ValueError, match=msg):
            t.tile_grid((128, 192), **kw)
    for canvas, bad in (((120, 192), 120), ((128, 180), 180)):
        with pytest.raises(ValueError, match="canvas sizes must be multiples of 32 \\(got %d\\)" % bad):
            t.tile_grid(canvas, (64, 96), 32, 8)
    assert t.check_args((64, 96)) == ((64, 96), 256, 32), "defaults: halo 256, blend 32"
    with pytest.raises(AssertionError, match="one array per tile"):
        t.stitch_host([], t.tile_grid((128, 192), (64, 96), 32, 8))


def test_refusals_before_anything_is_allocated():
    import torch
    from models.superslomo_r import FullModel
    from ssm_amd.config import load_config, synthetic_weight_overrides
    from ssm_amd.engine import PairPipeline, TiledEngine
    from ssm_amd.video import VideoInterpolator
    dev = torch.device("cpu")
    with pytest.raises(NotImplementedError, match=r"graphs=True\) does not cover tile=64x96"):
        PairPipeline({}, {}, 3, 128, 192, dev, graphs=True, tile=(64, 96), halo=32)
    with pytest.raises(NotImplementedError, match="tile=64x96 together with flow_scale=2"):
        PairPipeline({}, {}, 3, 128, 192, dev, flow_scale=2, tile=(64, 96), halo=32)
    with pytest.raises(ValueError, match="blend must be 0 or a power of two"):
        PairPipeline({}, {}, 3, 128, 192, dev, tile=(64, 96), halo=32, blend=3)
    with pytest.raises(AssertionError, match="covers the canvas is the plain PairEngine"):
        TiledEngine({}, {}, 1, 3, 128, 192, dev, (128, 192), 32, 8)
    cfg = load_config("superslomo_original.ini", synthetic_weight_overrides())
    with pytest.raises(ValueError, match="halo must be a multiple of 32"):
        VideoInterpolator(None, cfg, tile=(64, 96), halo=40)
    with pytest.raises(NotImplementedError, match="tile=64x96 together with flow_scale=4"):
        VideoInterpolator(None, cfg, tile=(64, 96), halo=32, flow_scale=4)
    fm = FullModel(cfg)
    assert fm._tile(None, 256, 32, 1) is None and fm._tile((64, 96), 32, 8, 1) == ((64, 96), 32, 8)
    with pytest.raises(NotImplementedError, match="tile=64x96 together with flow_scale=2"):
        fm._tile((64, 96), 32, 8, 2)
    rec = FullModel(load_config("superslomo_recurrent.ini", synthetic_weight_overrides()))
    with pytest.raises(NotImplementedError, match="tile=64x96 is not available with a recurrent bottleneck"):
        rec._tile((64, 96), 32, 8, 1)
    with pytest.raises(NotImplementedError, match="recurrent bottleneck"):
        VideoInterpolator(rec, cfg, tile=(64, 96), halo=32)


def test_cli_flags():
    import interpolate_video
    import visualize_interpolation
    base = ["-c", "x.ini", "--expt", "e", "--log", "l"]
    vid = base + ["--input", "-", "--output", "-"]
    vis = base + ["--input_dir", "i", "--img_type", "png", "--output_dir", "o"]
    for cli, argv in ((interpolate_video, vid), (visualize_interpolation, vis)):
        a = cli.getargs(argv)
        assert a.tile is None and (a.halo, a.blend) == (256, 32)
        a = cli.getargs(argv + ["--tile", "1088x1920"])
        assert a.tile == (1088, 1920) and (a.halo, a.blend) == (256, 32)
        a = cli.getargs(argv + ["--tile", "64x96", "--halo", "32", "--blend", "8"])
        assert (a.tile, a.halo, a.blend) == ((64, 96), 32, 8)
        for bad in ("1088", "1088x", "x1920", "1088x1920x3", "axb"):
            with pytest.raises(SystemExit):
                cli.getargs(argv + ["--tile", bad])


def test_visualizer_refuses_tiles_with_intermediate_outputs(tmp_path):
    import visualize_interpolation as vz
    from ssm_amd.config import load_config, synthetic_weight_overrides
    cfg = load_config("superslomo_original.ini", synthetic_weight_overrides())
    args = vz.getargs(["-c", "x.ini", "--expt", "e", "--log", "l", "--input_dir", "i", "--img_type", "png", "--output_dir", str(tmp_path),
                       "--tile", "64x96", "--halo", "32", "--show_intermediate_outputs"])

    class Stub:
        def cuda(self):
            return self

        def eval(self):
            return self
    with pytest.raises(NotImplementedError, match="--tile 64x96 with --show_intermediate_outputs"):
        vz.Interpolator(cfg, args, model=Stub())
