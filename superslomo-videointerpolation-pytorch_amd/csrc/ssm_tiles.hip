// Tiled inference (ssm_amd/tiles.py spells the geometry on the host): one tile's frames [N,C,window_h,window_w] are stitched
// into the full-size frames [N,C,Hp,Wp] with a cross-fade over the seams.  A launch writes the tile's region of influence - its core
// grown by b across every side that has a neighbour, inside the canvas - and nothing else.  Per pixel of it:
//     w = wy * wx,   p = w * v,   out = first ? p : out + p
// with the 1-D weights of include/ssm_hip.h (ssm_tile_stitch_fwd) computed from the coordinates - no table in memory - and `first` =
// the pixel lies in neither the tile's left band nor its top band: with the tiles visited in raster order, that tile is the first to
// cover the pixel, so the output needs no zero-fill and a later tile finds a stored value to add to.  Outside the bands w = 1 and the
// pixel is a plain copy.
// NO CONTRACTION, as in ssm_video.hip and ssm_flow.hip: the kernel is held bit for bit to a numpy yardstick that rounds every operation
// (ssm_amd.tiles.stitch_host), and hipcc would fuse out + w * v into one fma.  Off for the whole file by the pragma below.
// HBM-bound: 4 C bytes read and 4 C written per pixel and frame, plus the read-modify-write in the bands.  One lane = 4 consecutive
// pixels of one row (16-byte loads and stores; band edges are multiples of 4 because cores are multiples of 32 and b >= 4) for all C
// channels; views that are not 16-byte aligned take one pixel per lane.
#include "ssm_common.h"
#include "ssm_device.h"

#pragma clang fp contract(off)

namespace {

struct StitchParams {
    ssm_view tile, out;
    int C;
    int oy, ox;                       // window origin in the canvas
    int ry0, rx0, ry1, rx1;           // region of influence
    int cy0, cx0, cy1, cx1;           // core
    int top, bottom, left, right;     // sides with a neighbour
    int b;
    float inv_span;                   // 1 / (2b): a power of two, the division of the definition is this product exactly
};

// weight of position x on an axis whose core is [c0, c1): rises over [c0 - b, c0 + b) when the tile has a neighbour before it, falls over
// [c1 - b, c1 + b) when it has one after it; every step exact in fp32 (small integers + 0.5, times a power of two)
__device__ __forceinline__ float axis_weight(int x, int c0, int c1, int rises, int falls, int b, float inv_span) {
    float w = 1.0f;
    if (b) {
        if (rises) w = w * fminf(fmaxf(((float)(x - c0 + b) + 0.5f) * inv_span, 0.0f), 1.0f);
        if (falls) w = w * (1.0f - fminf(fmaxf(((float)(x - c1 + b) + 0.5f) * inv_span, 0.0f), 1.0f));
    }
    return w;
}

template <int V>          // pixels per lane: 4 (float4 accesses) or 1
__global__ __launch_bounds__(256) void tile_stitch_kernel(const StitchParams p) {
    const int x = p.rx0 + (blockIdx.x * 64 + threadIdx.x) * V;
    const int y = p.ry0 + blockIdx.y * 4 + threadIdx.y;
    const int n = blockIdx.z;
    if (x >= p.rx1 || y >= p.ry1) return;
    const int b = p.b;
    // bands: the rising ones decide `first`; inside any of them the pixel is weighted (V = 4: band edges are multiples of 4, so the four
    // pixels of a lane agree on both)
    const bool in_top = p.top && y < p.cy0 + b, in_left = p.left && x < p.cx0 + b;
    const bool in_band = in_top || in_left || (p.bottom && y >= p.cy1 - b) || (p.right && x >= p.cx1 - b);
    const bool first = !(in_top || in_left);
    const float *src = p.tile.ptr + (long long)n * p.tile.sb + (long long)(y - p.oy) * p.tile.sh + (x - p.ox);
    float *dst = p.out.ptr + (long long)n * p.out.sb + (long long)y * p.out.sh + x;
    if (!in_band) {          // w == 1, and no earlier tile reaches here
        for (int c = 0; c < p.C; ++c, src += p.tile.sc, dst += p.out.sc) {
            if constexpr (V == 4)
                *reinterpret_cast<float4 *>(dst) = *reinterpret_cast<const float4 *>(src);
            else
                *dst = *src;
        }
        return;
    }
    const float wy = axis_weight(y, p.cy0, p.cy1, p.top, p.bottom, b, p.inv_span);
    if constexpr (V == 4) {
        const float w0 = wy * axis_weight(x, p.cx0, p.cx1, p.left, p.right, b, p.inv_span);
        const float w1 = wy * axis_weight(x + 1, p.cx0, p.cx1, p.left, p.right, b, p.inv_span);
        const float w2 = wy * axis_weight(x + 2, p.cx0, p.cx1, p.left, p.right, b, p.inv_span);
        const float w3 = wy * axis_weight(x + 3, p.cx0, p.cx1, p.left, p.right, b, p.inv_span);
        for (int c = 0; c < p.C; ++c, src += p.tile.sc, dst += p.out.sc) {
            const float4 v = *reinterpret_cast<const float4 *>(src);
            float4 r = make_float4(w0 * v.x, w1 * v.y, w2 * v.z, w3 * v.w);
            if (!first) {
                const float4 o = *reinterpret_cast<const float4 *>(dst);
                r = make_float4(o.x + r.x, o.y + r.y, o.z + r.z, o.w + r.w);
            }
            *reinterpret_cast<float4 *>(dst) = r;
        }
    } else {
        const float w = wy * axis_weight(x, p.cx0, p.cx1, p.left, p.right, b, p.inv_span);
        for (int c = 0; c < p.C; ++c, src += p.tile.sc, dst += p.out.sc) {
            float r = w * *src;
            if (!first) r = *dst + r;
            *dst = r;
        }
    }
}

inline bool view16(const ssm_view &v) { return ssm::aligned16(v.ptr) && v.sh % 4 == 0 && v.sc % 4 == 0 && v.sb % 4 == 0; }

}  // namespace

extern "C" int ssm_tile_stitch_fwd(ssm_view tile, ssm_view out, int N, int C, int window_h, int window_w, int Hp, int Wp, int oy, int ox,
                                   int cy0, int cx0, int cy1, int cx1, int seams, int b, void *stream) {
    SSM_REQUIRE(tile.ptr && out.ptr, "tile_stitch: null pointer");
    SSM_REQUIRE(N > 0 && C > 0 && N <= 65535, "tile_stitch: bad sizes N=%d C=%d", N, C);
    SSM_REQUIRE(b == 0 || (b >= 4 && b <= 1024 && (b & (b - 1)) == 0), "tile_stitch: blend must be 0 or a power of two in 4..1024 (got %d)", b);
    SSM_REQUIRE(seams >= 0 && seams < 16, "tile_stitch: seams is a mask of 4 sides (got %d)", seams);
    SSM_REQUIRE(Hp > 0 && Wp > 0 && window_h > 0 && window_w > 0 && Hp <= (1 << 24) && Wp <= (1 << 24),
                "tile_stitch: geometry: canvas %dx%d, window %dx%d", Hp, Wp, window_h, window_w);
    SSM_REQUIRE(oy >= 0 && ox >= 0 && window_h <= Hp - oy && window_w <= Wp - ox,
                "tile_stitch: geometry: window %dx%d at (%d, %d) outside the canvas %dx%d", window_h, window_w, oy, ox, Hp, Wp);
    SSM_REQUIRE(cy0 >= 0 && cx0 >= 0 && cy0 < cy1 && cx0 < cx1 && cy1 <= Hp && cx1 <= Wp,
                "tile_stitch: geometry: core rows [%d, %d) x columns [%d, %d) outside the canvas %dx%d", cy0, cy1, cx0, cx1, Hp, Wp);
    const int top = seams & 1, bottom = (seams >> 1) & 1, left = (seams >> 2) & 1, right = (seams >> 3) & 1;
    // the fade-in and fade-out bands of an axis must not meet, and a side with a neighbour is not a canvas edge
    SSM_REQUIRE((!(top && bottom) || 2 * b <= cy1 - cy0) && (!(left && right) || 2 * b <= cx1 - cx0),
                "tile_stitch: geometry: blend %d needs a core of at least %d between two seams (core %dx%d)", b, 2 * b, cy1 - cy0, cx1 - cx0);
    SSM_REQUIRE((!top || cy0 >= b) && (!left || cx0 >= b) && (!top || cy0 > 0) && (!left || cx0 > 0) && (!bottom || cy1 < Hp) && (!right || cx1 < Wp),
                "tile_stitch: geometry: a seam on a canvas edge (core rows [%d, %d) x columns [%d, %d), seams %d, canvas %dx%d)", cy0, cy1, cx0,
                cx1, seams, Hp, Wp);
    StitchParams p;
    p.tile = tile, p.out = out, p.C = C, p.oy = oy, p.ox = ox, p.b = b;
    p.cy0 = cy0, p.cx0 = cx0, p.cy1 = cy1, p.cx1 = cx1;
    p.top = top, p.bottom = bottom, p.left = left, p.right = right;
    p.inv_span = b ? 1.0f / (float)(2 * b) : 0.0f;
    p.ry0 = cy0 - (top ? b : 0), p.rx0 = cx0 - (left ? b : 0);
    p.ry1 = bottom ? (cy1 + b < Hp ? cy1 + b : Hp) : cy1;
    p.rx1 = right ? (cx1 + b < Wp ? cx1 + b : Wp) : cx1;
    SSM_REQUIRE(p.ry0 >= oy && p.rx0 >= ox && p.ry1 <= oy + window_h && p.rx1 <= ox + window_w,
                "tile_stitch: geometry: window %dx%d at (%d, %d) smaller than the core rows [%d, %d) x columns [%d, %d) grown by blend %d",
                window_h, window_w, oy, ox, cy0, cy1, cx0, cx1, b);
    const int rh = p.ry1 - p.ry0, rw = p.rx1 - p.rx0;
    SSM_REQUIRE((rh + 3) / 4 <= 65535, "tile_stitch: geometry: region of %d rows too tall for one launch", rh);
    const bool vec = view16(tile) && view16(out) && ox % 4 == 0 && p.rx0 % 4 == 0 && p.rx1 % 4 == 0 && cx0 % 4 == 0 && cx1 % 4 == 0;
    if (vec)
        SSM_LAUNCH(tile_stitch_kernel<4>, dim3((rw / 4 + 63) / 64, (rh + 3) / 4, N), dim3(64, 4), 0, (hipStream_t)stream, p);
    else
        SSM_LAUNCH(tile_stitch_kernel<1>, dim3((rw + 63) / 64, (rh + 3) / 4, N), dim3(64, 4), 0, (hipStream_t)stream, p);
    return ssm::check_launch("ssm_tile_stitch_fwd");
}
