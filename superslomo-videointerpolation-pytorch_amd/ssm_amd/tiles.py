"""Tiled inference (`tile = (th, tw)`): the frame runs through the U-Nets in overlapping windows, the windows' frames are stitched.

Beyond the reference's operator surface and an approximation of the untiled output, not parity: the U-Nets' receptive
field is wider than any practical halo.  This module holds what the engine, the tools and the tests share about the mode and needs no GPU:

  parse_tile     "HxW" of the command lines -> (th, tw)
  check_args     tile / halo / blend, refused by name
  axis_plan      cores, window length and window origins of one axis
  tile_grid      the tiles of a canvas in raster order (TileGrid / Tile)
  axis_weights   the 1-D cross-fade weights of a tile: the rule csrc/ssm_tiles.hip evaluates per lane
  stitch_host    float32 yardstick of ssm_tile_stitch_fwd: the kernel's rounded operations in the kernel's order

Per axis, with canvas length L, core size c and n = ceil(L / c): the cores [k c, min((k+1) c, L)) partition the canvas; every tile has the
same window length (L if n = 1, min(L, c + halo) if n = 2 - every tile then touches a canvas edge -, min(L, c + 2 halo) otherwise) so one
plan serves all tiles; the window of tile k starts at clamp(k c - halo, 0, L - window).  c and halo are multiples of 32, so every origin
is one and the tiles' pooling grids coincide with the untiled plan's.
"""
import collections
import re

import numpy as np

DEFAULT_HALO = 256       # SURVEY's figure for config 5; not backed by a measurement of quality
DEFAULT_BLEND = 32       # likewise
MAX_BLEND = 1024         # weights are odd multiples of 1/(4b): up to here their products, and 1 - a product, are exact in float32

# sides of a tile that are interior seams: the bits of ssm_tile_stitch_fwd's `seams`
SEAM_TOP, SEAM_BOTTOM, SEAM_LEFT, SEAM_RIGHT = 1, 2, 4, 8

Tile = collections.namedtuple("Tile", "ky kx y0 x0 cy0 cx0 cy1 cx1 seams")
Tile.__doc__ = """One tile: grid position (ky, kx), window origin (y0, x0), core rows [cy0, cy1) and columns [cx0, cx1) in canvas
coordinates, `seams` = the SEAM_* bits of its sides that have a neighbour."""


def parse_tile(text):
    """"1088x1920" -> (1088, 1920); anything else is a ValueError naming the text (argparse reports it as a usage error)."""
    m = re.fullmatch(r"(\d+)[xX](\d+)", str(text).strip())
    if not m:
        raise ValueError("tile must be written HxW, e.g. 1088x1920 (got %r)" % (text,))
    return int(m.group(1)), int(m.group(2))


def check_args(tile, halo=DEFAULT_HALO, blend=DEFAULT_BLEND):
    """(th, tw), halo, blend as ints; what the geometry does not accept is refused by name."""
    try:
        th, tw = tile
        th, tw = int(th), int(tw)
    except (TypeError, ValueError):
        raise ValueError("tile must be a pair (th, tw) of core sizes (got %r)" % (tile,)) from None
    for name, c in (("tile height", th), ("tile width", tw)):
        if c < 64 or c % 32:
            raise ValueError("%s must be a multiple of 32 and at least 64 (got %d)" % (name, c))
    if int(halo) != halo or halo < 32 or halo % 32:
        raise ValueError("halo must be a multiple of 32 and at least 32 (got %r)" % (halo,))
    b = blend
    if int(b) != b or b < 0 or (b != 0 and (b < 4 or b & (b - 1))):
        raise ValueError("blend must be 0 or a power of two >= 4 (got %r)" % (b,))
    if b > halo:
        raise ValueError("blend must not exceed the halo (got blend %d > halo %d)" % (b, halo))
    if b > MAX_BLEND:
        raise ValueError("blend must not exceed %d, where the cross-fade weights stop being exact in float32 (got %d)" % (MAX_BLEND, b))
    if 2 * b > min(th, tw):
        raise ValueError("the cross-fade bands of a tile must not meet: 2 * blend <= tile size (got blend %d, tile %dx%d)" % (b, th, tw))
    return (th, tw), int(halo), int(b)


def axis_plan(L, c, halo):
    """(window length, [(core start, core end, window origin)] for the n = ceil(L / c) tiles of one axis)."""
    if L < 32 or L % 32:
        raise ValueError("canvas sizes must be multiples of 32 (got %d)" % L)
    n = -(-L // c)
    window = L if n == 1 else min(L, c + halo) if n == 2 else min(L, c + 2 * halo)
    return window, [(k * c, min((k + 1) * c, L), min(max(k * c - halo, 0), L - window)) for k in range(n)]


class TileGrid:
    """The tiles of an (Hp, Wp) canvas in raster order.  Attributes: canvas, tile, halo, blend, ny, nx, window = (window_h, window_w),
    tiles (list of Tile)."""

    def __init__(self, canvas, tile, halo=DEFAULT_HALO, blend=DEFAULT_BLEND):
        self.tile, self.halo, self.blend = check_args(tile, halo, blend)
        self.canvas = Hp, Wp = int(canvas[0]), int(canvas[1])
        wh, ys = axis_plan(Hp, self.tile[0], self.halo)
        ww, xs = axis_plan(Wp, self.tile[1], self.halo)
        self.window, self.ny, self.nx = (wh, ww), len(ys), len(xs)
        self.tiles = []
        for ky, (cy0, cy1, y0) in enumerate(ys):
            for kx, (cx0, cx1, x0) in enumerate(xs):
                seams = ((SEAM_TOP if ky > 0 else 0) | (SEAM_BOTTOM if ky < self.ny - 1 else 0)
                         | (SEAM_LEFT if kx > 0 else 0) | (SEAM_RIGHT if kx < self.nx - 1 else 0))
                self.tiles.append(Tile(ky, kx, y0, x0, cy0, cx0, cy1, cx1, seams))

    def __len__(self):
        return len(self.tiles)

    def region(self, t):
        """(ry0, ry1, rx0, rx1): the tile's region of influence - its core grown by `blend` across each interior seam, inside the canvas."""
        b, (Hp, Wp) = self.blend, self.canvas
        return (t.cy0 - (b if t.seams & SEAM_TOP else 0), min(t.cy1 + (b if t.seams & SEAM_BOTTOM else 0), Hp),
                t.cx0 - (b if t.seams & SEAM_LEFT else 0), min(t.cx1 + (b if t.seams & SEAM_RIGHT else 0), Wp))


def tile_grid(canvas, tile, halo=DEFAULT_HALO, blend=DEFAULT_BLEND):
    return TileGrid(canvas, tile, halo, blend)


def covers_canvas(canvas, tile):
    """A tile at least as large as the canvas on both axes: one window, the canvas itself - the plain engine, not a tiled one."""
    return tile[0] >= canvas[0] and tile[1] >= canvas[1]


def axis_weights(lo, hi, c0, c1, rises, falls, b):
    """float32 weights of a tile over canvas positions lo .. hi - 1 of one axis, and which of them lie in its rising band.  The tile's
    core is [c0, c1); `rises`: it has a neighbour before c0 and fades in over [c0 - b, c0 + b) as u(x) = clamp((x - c0 + b + 0.5) / (2b), 0, 1);
    `falls`: it has one after c1 and fades out as 1 - u(x) around c1.  2b <= c keeps the two bands apart, so one factor is always 1.
    b = 0: a step at the seam (weight 1 over the core)."""
    x = np.arange(lo, hi, dtype=np.float32)
    one, zero = np.float32(1.0), np.float32(0.0)
    w = np.ones(hi - lo, dtype=np.float32)
    rising = np.zeros(hi - lo, dtype=bool)
    if b:
        bf, half, span = np.float32(b), np.float32(0.5), np.float32(2 * b)
        if rises:
            w = w * np.minimum(np.maximum((x - np.float32(c0) + bf + half) / span, zero), one)
            rising = np.arange(lo, hi) < c0 + b
        if falls:
            w = w * (one - np.minimum(np.maximum((x - np.float32(c1) + bf + half) / span, zero), one))
    return w.astype(np.float32), rising


def tile_weights(grid, t):
    """(w [rh, rw] float32, first [rh, rw] bool) over the tile's region of influence: a pixel's weight is the product of its two 1-D
    weights; `first`: this tile is the first in raster order to cover the pixel (it lies in neither the tile's left nor its top band)."""
    ry0, ry1, rx0, rx1 = grid.region(t)
    wy, top = axis_weights(ry0, ry1, t.cy0, t.cy1, t.seams & SEAM_TOP, t.seams & SEAM_BOTTOM, grid.blend)
    wx, left = axis_weights(rx0, rx1, t.cx0, t.cx1, t.seams & SEAM_LEFT, t.seams & SEAM_RIGHT, grid.blend)
    return wy[:, None] * wx[None, :], ~(top[:, None] | left[None, :])


def stitch_host(tiles, grid, out=None):
    """numpy float32 yardstick of ssm_tile_stitch_fwd over a whole grid.  tiles: one [N,C,window_h,window_w] array per tile of `grid`,
    raster order.  Returns [N,C,Hp,Wp] (`out` if given; else a NaN-filled array, so a pixel nobody stored shows).  Per tile and pixel
    of its region of influence: p = w * v (rounded); the first tile to cover the pixel stores p, every later one out + p (rounded)."""
    assert len(tiles) == len(grid), "one array per tile: %d given, the grid has %d" % (len(tiles), len(grid))
    first_tile = np.asarray(tiles[0])
    if out is None:
        out = np.full(first_tile.shape[:2] + grid.canvas, np.nan, dtype=np.float32)
    for t, v in zip(grid.tiles, tiles):
        v = np.asarray(v, dtype=np.float32)
        assert v.shape[2:] == grid.window, "tile of %s for windows of %s" % (v.shape[2:], grid.window)
        ry0, ry1, rx0, rx1 = grid.region(t)
        w, first = tile_weights(grid, t)
        p = w * v[:, :, ry0 - t.y0:ry1 - t.y0, rx0 - t.x0:rx1 - t.x0]
        dst = out[:, :, ry0:ry1, rx0:rx1]
        with np.errstate(invalid="ignore"):
            dst[...] = np.where(first, p, dst + p)
    return out
