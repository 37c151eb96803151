// Planar Y'CbCr video frames <-> the path's normalised, padded fp32 planes: the two conversions either side of the streamed
// video loop (ssm_amd/video.py), next to frames_from_u8_kernel / frames_to_u8_kernel of ssm_elem.hip, whose geometry (centred pad to
// x32, pad_before_norm in both conventions: scripts/visualize_interpolation.py:61-88, scripts/utils/dataloaders/augmentations.py:
// 141-200) and whose normalise / denormalise expressions they keep.  A frame is the payload of a YUV4MPEG2 FRAME record: the Y plane
// H x W, then U, then V, each ceil(H/2) x ceil(W/2) (4:2:0), H x ceil(W/2) (4:2:2) or H x W (4:4:4), no row padding; N frames are
// contiguous.  A sample is one byte, or (9 to 16 significant bits) a 16-bit little-endian word with the value in its low bits: the
// sample type and the layout are the kernels' template parameters, the bit depth lives in the constant table alone.
//   frames_from_yuv_kernel   one thread per 2 x 2 luma block: 3 x 3 chroma samples per plane (clamped at the edges) give the block's
//                            four bilinearly upsampled chroma values; range, matrix, clamp, normalise; two floats per row and plane
//                            go out as one 8-byte store when the view allows it
//   frames_to_yuv_kernel     one thread per 4 x 2 luma block = two chroma samples: denormalise, matrix, chroma filtered and subsampled
//                            in float, range, round half to even, saturate; four Y codes of a row go out as one store (4 or 8 bytes),
//                            the two chroma codes of a plane and row as one store (2 or 4 bytes), when size and alignment allow it
//   frames_accumulate_kernel the shutter of the streamed loop: N frames summed, in increasing n, into one fp32 accumulator
//                            that is read at most once and written once per launch; one lane = 4 consecutive pixels of a row of one
//                            channel (16-byte loads and stores), or one pixel when a view does not allow it.  Two modes: the
//                            sum of the coded values as they are, or the sum taken in light - every value denormalised, clamped to [0, 1]
//                            and decoded by one of the light curves of ssm_amd.video.light_curve before it is added, the mean encoded and
//                            normalised again by the call that closes an output; the power is v_log_f32, a multiply and v_exp_f32
//   frames_accumulate_hdr_kernel  the same skeleton (accumulate_lane) with the transfer functions of HDR clips in place of a light curve: the
//                            BT.2100 PQ EOTF and the inverse HLG OETF and their inverses, by v_log_f32, v_exp_f32, v_rcp_f32, v_sqrt_f32
//   frames_accumulate_weighted_kernel / frames_accumulate_hdr_weighted_kernel  the shutter windows: the two kernels above with a weight per
//                            frame, multiplied into the decoded sample before it is added (accumulate_lane<.., Weighted = true>); at most
//                            SSM_ACC_WEIGHTS_MAX weights, by value in the kernel's arguments, read as scalar operands
//   span_sum_kernel          the sums over pairs of payloads, one kernel under two entry points: per pair and plane the exact sum of a
//                            lane accumulator's term over the samples as they stand in the payloads.  A workgroup sums SPAN_BYTES = 16 KiB of
//                            ONE plane, a lane CHUNKS = 4 pieces of 16 bytes per operand (one 16-byte load each; sample by sample where a
//                            plane does not start on a 16-byte boundary and at a plane's ragged end); workgroup_add closes it: shuffles, LDS
//                            partials, one 64-bit atomic per workgroup.  PlaneOf turns the grid's x index into (plane, workgroup within it).
//                              SadLane      scene cuts, ssm_luma_sad_fwd: |a - b| over the 8-bit Y plane alone (one plane per payload), four
//                                           bytes per v_sad_u8 into a 32-bit lane sum
//                              SseLane<S>   hold-out scoring, ssm_plane_sse_fwd: (a - b)^2 over Y, U and V, 8-bit or 16-bit; bytes through
//                                           v_dot4_u32_u8 into 32-bit lane sums, words into 64-bit ones
//   field_diff_kernel        pulldown removal, ssm_field_diff_fwd: |a - b| over a luma plane summed per ROW PARITY, the differences of the top
//                            and of the bottom fields of two frames; the same workgroup and lane work walked by rows (FieldWalk), bytes
//                            through v_sad_u8 (SadLane), words through v_sad_u16 (SadWordLane), two 64-bit atomics per workgroup
//   field_order_sums_kernel  field order from the data, ssm_field_order_sums_fwd: per frame the comb sums A0, A1, D of its luma plane against the
//                            frame before and the frame after, |c[y-1] + c[y+1] - 2 r[y]| for r = p, n, c; a lane owns a 16-byte column piece
//                            and walks a band of rows with three rows of c in registers, bytes as packed 16-bit pairs through v_sad_u16,
//                            words in 32 bits, three 64-bit atomics per workgroup
//   plane_ssim_kernel        hold-out scoring: per frame pair and plane the SSIM of x264 / ffmpeg's ssim filter in fixed point - 4 x 4 block
//                            sums (bytes through v_dot4_u32_u8) to LDS, 8 x 8 windows at stride 4 from four blocks, integer factors, one
//                            float64 quotient per window rounded to a multiple of 2^-32, signed 64-bit sums; a workgroup owns 31 x 15 windows
//                            of one plane (PlaneOf) and ends in workgroup_add
//   block_sad_kernel         repeated frames, ssm_block_sad_fwd: |a - b| summed per 8 x 8 block of Y, U and V, per pair and plane the largest
//                            block sum and the number of blocks above `lo`; a workgroup owns 32 x 8 blocks of one plane (PlaneOf), a lane
//                            one block - eight 8- or 16-byte loads per operand, v_sad_u8 / v_sad_u16 - and ends in one 64-bit atomicMax and
//                            one 64-bit atomicAdd
//   static_paste_kernel      blocks that do not change, ssm_static_paste_fwd: |a - b| summed per 8 x 8 block of the FRAME - its luma and the U and V
//                            samples under it - and where the sum is at most `lo` the block's samples of `a` stored into the T outputs of the
//                            pair; a workgroup owns 256 blocks, 32 at a time, 8 neighbouring lanes a block, a lane one luma row and its share of the
//                            chroma rows (one load per piece where its address allows); shuffles, then one 64-bit atomicAdd of the count
//   flow_paste_kernel        the flow check's per-block fallback, ssm_flow_paste_fwd: per 8 x 8 block the luma positions that the pair's two mask
//                            planes call inconsistent, pop-counted, and where they are more than K the block's samples of the nearer frame
//                            stored into the pair's outputs (a below `split`, b from there on); static_paste_kernel's strips, lanes and pieces
//   payload_mix_kernel       hold-out scoring: the cross-fade (a (den - k) + b k + den / 2) / den of two payloads, the frame-blend baseline;
//                            exact division by multiply-shift, the span walk's pieces with a 16-byte store in place of the sum
//   flow_mix_kernel          the per-block fallback as a cross-fade, ssm_flow_mix_fwd: flow_paste_kernel's blocks, measure (flow_block_bad) and
//                            count; where a block fails, its pieces of a AND of b loaded once and payload_mix_kernel's exact mix of them
//                            (mix_word) stored into every output of the pair under that output's weights
//   fields_split_kernel /    interlaced clips: N frames -> their 2N fields (even rows of every plane, odd rows), and N fields with
//   fields_weave_kernel      N synthesised fields (or, fill = 1, with integer line averages of the kept field itself) -> N frames; bytes moved
//                            as they stand, 16-byte pieces of a row where the addresses allow, one launch for the three planes
//   luma_counts_kernel       letterboxed clips, ssm_luma_counts_fwd: per frame the luma samples above a limit of every row and of every column; a
//                            workgroup owns 256 columns x 32 rows, a lane four columns, a wave every fourth row; shuffles and LDS, then one
//                            32-bit atomic per row and column tile and one per column and band
//   window_cut_kernel        letterboxed clips, ssm_window_cut_fwd: the window of a rectangle of N payloads as packed payloads, the field
//                            kernels' 16-byte pieces walked over the window's rows of the three planes
// On the host the six pair entry points share pair_given and check_pair (operands, strides, alignment), grid_fits and clear_sums; yuv_planes is the one
// place that knows the plane sizes of 4:2:0, 4:2:2 and 4:4:4, with_layout and with_sample pick a kernel's two template parameters.
// Both conversions are HBM-bound (1.5 to 6 B in + 12 B out per pixel, and the reverse); so is the accumulation (4 (N + 1 + !init) B per
// element), the luma difference (2 B per pixel) and the squared differences (2 B per pair of samples).  The chroma siting enters as four horizontal weights (ingest) or one switch (egress); matrix and range enter as one row of
// the constant table built by ssm_amd/video.py, which the host yardsticks read too.  Inputs of the egress kernel are finite.
// NO CONTRACTION (as ssm_flow.hip): the numpy yardsticks round every operation, and so must the kernels.
#include "ssm_common.h"
#include "ssm_device.h"

#include <cmath>
#include <cstdlib>

#pragma clang fp contract(off)

namespace {

// one row of the constant table (include/ssm_hip.h: SSM_YUV_ROW floats per (matrix, range))
struct YuvRow {
    float kr, kg, kb;            // luma weights
    float rv, gu, gv, bu;        // Y'CbCr -> R'G'B'
    float cbs, crs;              // 1 / (2 (1 - Kb)), 1 / (2 (1 - Kr))
    float ys, cs;                // code -> full scale: 255/219, 255/224 (limited) or 1
    float iys, ics;              // full scale -> code: 219/255, 224/255 or 1
    float yoff, coff;            // 16 | 0, 128
    float ylo, yhi, clo, chi;    // saturation bounds of the codes
    float reserved;
};
static_assert(sizeof(YuvRow) == SSM_YUV_ROW * sizeof(float), "table row");

struct Norm3 {
    float m[3], s[3];
};

__device__ __forceinline__ float *vp(const ssm_view &v, int b, int c, int y) {
    return v.ptr + (long long)b * v.sb + (long long)c * v.sc + (long long)y * v.sh;
}

__device__ __forceinline__ float clampf(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }

// ---- ingest ------------------------------------------------------------------------------------------------------------------------
// wx = {a0, a1, b1, b2}: chroma at an even luma column 2j = a0 c[j-1] + a1 c[j], at an odd one = b1 c[j] + b2 c[j+1]
// (centred siting .25 .75 .75 .25; co-sited with the even columns 0 1 .5 .5).  Rows are centred in both sitings.
// Thread (bx, by) owns the luma block at source (2 by - T2, 2 bx - L2), T2 / L2 = top / left rounded up to even, so that blocks are
// aligned with the chroma grid wherever the image sits in the canvas; canvas pixels outside the image get the pad value.
// 4:2:2 takes the horizontal step alone (wx that of the co-sited case), on the luma row's own chroma row.
enum { LAY_420 = 0, LAY_422 = 1, LAY_444 = 2 };          // the plane layouts a kernel is instantiated for

template <typename S, int L>          // S: the sample, unsigned char or unsigned short
__global__ __launch_bounds__(256) void frames_from_yuv_kernel(const S *__restrict__ in, ssm_view out, int H, int W, int Hp, int Wp,
                                                              int top, int left, long long frame_samples, YuvRow k, Norm3 nm, float a0,
                                                              float a1, float b1, float b2, int pad_before_norm, int vec2) {
    const int bx = blockIdx.x * 64 + threadIdx.x, by = blockIdx.y * 4 + threadIdx.y, b = blockIdx.z;
    const int sx0 = 2 * bx - ((left + 1) & ~1), sy0 = 2 * by - ((top + 1) & ~1);          // source position of the block
    const int ox0 = sx0 + left, oy0 = sy0 + top;                                         // canvas position (-1 possible)
    if (ox0 >= Wp || oy0 >= Hp) return;
    const int cw = L == LAY_444 ? W : (W + 1) >> 1, ch = L == LAY_420 ? (H + 1) >> 1 : H;
    const S *yp = in + (long long)b * frame_samples;
    const S *up = yp + (long long)H * W, *vpl = up + (long long)ch * cw;
    float o[3][2][2];          // [plane][row][col]
    const bool any = sx0 + 1 >= 0 && sx0 < W && sy0 + 1 >= 0 && sy0 < H;
    float cu[2][2], cv[2][2];  // upsampled chroma of the block
    if (any) {
        if (L == LAY_444) {
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const int y = min(max(sy0 + r, 0), H - 1), x = min(max(sx0 + c, 0), W - 1);
                    cu[r][c] = (float)up[(long long)y * W + x];
                    cv[r][c] = (float)vpl[(long long)y * W + x];
                }
        } else if (L == LAY_422) {
            const int j = sx0 >> 1;          // sx0 even (arithmetic shift: -2 -> -1)
            int xs[3];
#pragma unroll
            for (int t = 0; t < 3; ++t) xs[t] = min(max(j - 1 + t, 0), cw - 1);
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int y = min(max(sy0 + r, 0), H - 1);
                const S *ur = up + (long long)y * cw, *vr = vpl + (long long)y * cw;
                const float u0 = (float)ur[xs[0]], u1 = (float)ur[xs[1]], u2 = (float)ur[xs[2]];
                const float v0 = (float)vr[xs[0]], v1 = (float)vr[xs[1]], v2 = (float)vr[xs[2]];
                cu[r][0] = a0 * u0 + a1 * u1;
                cu[r][1] = b1 * u1 + b2 * u2;
                cv[r][0] = a0 * v0 + a1 * v1;
                cv[r][1] = b1 * v1 + b2 * v2;
            }
        } else {
            const int j = sx0 >> 1, i = sy0 >> 1;          // sx0, sy0 even (arithmetic shift: -2 -> -1)
            int xs[3], ys[3];
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                xs[t] = min(max(j - 1 + t, 0), cw - 1);
                ys[t] = min(max(i - 1 + t, 0), ch - 1);
            }
            float hu[3][2], hv[3][2];          // horizontally interpolated: [chroma row][even | odd luma column]
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const S *ur = up + (long long)ys[r] * cw, *vr = vpl + (long long)ys[r] * cw;
                const float u0 = (float)ur[xs[0]], u1 = (float)ur[xs[1]], u2 = (float)ur[xs[2]];
                const float v0 = (float)vr[xs[0]], v1 = (float)vr[xs[1]], v2 = (float)vr[xs[2]];
                hu[r][0] = a0 * u0 + a1 * u1;
                hu[r][1] = b1 * u1 + b2 * u2;
                hv[r][0] = a0 * v0 + a1 * v1;
                hv[r][1] = b1 * v1 + b2 * v2;
            }
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                cu[0][c] = 0.25f * hu[0][c] + 0.75f * hu[1][c];
                cu[1][c] = 0.75f * hu[1][c] + 0.25f * hu[2][c];
                cv[0][c] = 0.25f * hv[0][c] + 0.75f * hv[1][c];
                cv[1][c] = 0.75f * hv[1][c] + 0.25f * hv[2][c];
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int sy = sy0 + r, sx = sx0 + c;
            const bool inside = any && sy >= 0 && sy < H && sx >= 0 && sx < W;
            if (inside) {
                const float yl = ((float)yp[(long long)sy * W + sx] - k.yoff) * k.ys;
                const float cb = (cu[r][c] - k.coff) * k.cs, cr = (cv[r][c] - k.coff) * k.cs;
                float rgb[3];
                rgb[0] = yl + k.rv * cr;
                rgb[1] = (yl - k.gu * cb) - k.gv * cr;
                rgb[2] = yl + k.bu * cb;
#pragma unroll
                for (int p = 0; p < 3; ++p) o[p][r][c] = (clampf(rgb[p], 0.0f, 255.0f) / 255.0f - nm.m[p]) / nm.s[p];
            } else {
#pragma unroll
                for (int p = 0; p < 3; ++p) o[p][r][c] = pad_before_norm ? (0.0f / 255.0f - nm.m[p]) / nm.s[p] : 0.0f;
            }
        }
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int oy = oy0 + r;
            if (oy < 0 || oy >= Hp) continue;
            float *row = vp(out, b, p, oy);
            if (vec2 && ox0 + 1 < Wp) {          // vec2: left even (ox0 >= 0 and even), 8-byte aligned view
                f32x2 v;
                v.x = o[p][r][0];
                v.y = o[p][r][1];
                *reinterpret_cast<f32x2 *>(row + ox0) = v;
            } else {
                if (ox0 >= 0) row[ox0] = o[p][r][0];
                if (ox0 + 1 < Wp) row[ox0 + 1] = o[p][r][1];
            }
        }
}

// ---- egress ------------------------------------------------------------------------------------------------------------------------
// Thread (bx, by) owns the luma block at (2 by, 4 bx) of the H x W crop.  Columns / rows past the crop (odd sizes) repeat the last one.
struct Ycc {
    float y, cb, cr;
};
__device__ __forceinline__ Ycc to_ycc(float r, float g, float b, const YuvRow &k) {
    Ycc o;
    o.y = (k.kr * r + k.kg * g) + k.kb * b;
    o.cb = (b - o.y) * k.cbs;
    o.cr = (r - o.y) * k.crs;
    return o;
}
__device__ __forceinline__ float denorm(float v, float sd, float mean) {
    float t = v * sd + mean;
    t = t * 255.0f;
    return t;
}
__device__ __forceinline__ unsigned code_of(float v, float scale, float off, float lo, float hi) {
    return (unsigned)(int)clampf(rintf(v * scale + off), lo, hi);
}

// four codes of a row / two chroma codes of a plane as one store: 4 and 2 bytes of 8-bit samples, 8 and 4 bytes of 16-bit ones
__device__ __forceinline__ void store4(unsigned char *dst, const unsigned (&q)[4]) {
    *reinterpret_cast<unsigned *>(dst) = q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24);
}
__device__ __forceinline__ void store4(unsigned short *dst, const unsigned (&q)[4]) {
    i32x2 v;
    v.x = (int)(q[0] | (q[1] << 16));
    v.y = (int)(q[2] | (q[3] << 16));
    *reinterpret_cast<i32x2 *>(dst) = v;
}
__device__ __forceinline__ void store2(unsigned char *dst, unsigned q0, unsigned q1) {
    *reinterpret_cast<unsigned short *>(dst) = (unsigned short)(q0 | (q1 << 8));
}
__device__ __forceinline__ void store2(unsigned short *dst, unsigned q0, unsigned q1) { *reinterpret_cast<unsigned *>(dst) = q0 | (q1 << 16); }

template <typename S, int L>
__global__ __launch_bounds__(256) void frames_to_yuv_kernel(ssm_view in, S *__restrict__ out, int H, int W, int top, int left,
                                                            long long frame_samples, YuvRow k, Norm3 nm, int cosited, int vec_in, int vec_out) {
    const int bx = blockIdx.x * 64 + threadIdx.x, by = blockIdx.y * 4 + threadIdx.y, b = blockIdx.z;
    const int x0 = 4 * bx, y0 = 2 * by;
    if (x0 >= W || y0 >= H) return;
    const int cw = L == LAY_444 ? W : (W + 1) >> 1, ch = L == LAY_420 ? (H + 1) >> 1 : H;
    const bool cos = L == LAY_422 || (L == LAY_420 && cosited);          // 4:2:2 is co-sited with the even luma columns
    S *yp = out + (long long)b * frame_samples;
    S *up = yp + (long long)H * W, *vpl = up + (long long)ch * cw;
    const bool whole = x0 + 3 < W;
    Ycc px[2][5];          // [row][column x0-1 (co-sited only), x0 .. x0+3]
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int y = min(y0 + r, H - 1) + top;
        float v[3][5];
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            const float *row = vp(in, b, p, y) + left;
            if (vec_in && whole) {          // vec_in: 16-byte aligned rows at x0
                const f32x4 q = *reinterpret_cast<const f32x4 *>(row + x0);
                v[p][1] = q.x, v[p][2] = q.y, v[p][3] = q.z, v[p][4] = q.w;
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c) v[p][1 + c] = row[min(x0 + c, W - 1)];
            }
            v[p][0] = cos ? row[max(x0 - 1, 0)] : 0.0f;
        }
#pragma unroll
        for (int c = 0; c < 5; ++c)
            px[r][c] = to_ycc(denorm(v[0][c], nm.s[0], nm.m[0]), denorm(v[1][c], nm.s[1], nm.m[1]), denorm(v[2][c], nm.s[2], nm.m[2]), k);
    }
    // luma (and, 4:4:4, chroma) codes: four per row
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int y = y0 + r;
        if (y >= H) continue;
#pragma unroll
        for (int p = 0; p < (L == LAY_444 ? 3 : 1); ++p) {
            unsigned q[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const Ycc &s = px[r][1 + c];
                q[c] = p == 0 ? code_of(s.y, k.iys, k.yoff, k.ylo, k.yhi) : code_of(p == 1 ? s.cb : s.cr, k.ics, k.coff, k.clo, k.chi);
            }
            S *dst = (p == 0 ? yp : (p == 1 ? up : vpl)) + (long long)y * W + x0;
            if (vec_out && whole) {          // vec_out: W % 4 == 0 and planes aligned to four samples
                store4(dst, q);
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (x0 + c < W) dst[c] = (S)q[c];
            }
        }
    }
    if (L == LAY_444) return;
    // the block's two chroma samples - per row in 4:2:2: filter in float, then range, rounding, saturation
#pragma unroll
    for (int cr_ = 0; cr_ < (L == LAY_422 ? 2 : 1); ++cr_) {
        if (L == LAY_422 && y0 + cr_ >= H) continue;
        unsigned qu[2], qv[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int c = 1 + 2 * j;          // px column of luma column 2 (cx) = x0 + 2 j
            float cb, cr;
            if (L == LAY_422) {               // [1 2 1] / 4 over columns 2 cx - 1 .. 2 cx + 1 of the row itself
                cb = ((px[cr_][c - 1].cb + 2.0f * px[cr_][c].cb) + px[cr_][c + 1].cb) * 0.25f;
                cr = ((px[cr_][c - 1].cr + 2.0f * px[cr_][c].cr) + px[cr_][c + 1].cr) * 0.25f;
            } else if (cosited) {             // the same, then the mean of the two rows
                float hb[2], hr[2];
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    hb[r] = ((px[r][c - 1].cb + 2.0f * px[r][c].cb) + px[r][c + 1].cb) * 0.25f;
                    hr[r] = ((px[r][c - 1].cr + 2.0f * px[r][c].cr) + px[r][c + 1].cr) * 0.25f;
                }
                cb = (hb[0] + hb[1]) * 0.5f;
                cr = (hr[0] + hr[1]) * 0.5f;
            } else {                          // 2 x 2 mean
                cb = ((px[0][c].cb + px[0][c + 1].cb) + (px[1][c].cb + px[1][c + 1].cb)) * 0.25f;
                cr = ((px[0][c].cr + px[0][c + 1].cr) + (px[1][c].cr + px[1][c + 1].cr)) * 0.25f;
            }
            qu[j] = code_of(cb, k.ics, k.coff, k.clo, k.chi);
            qv[j] = code_of(cr, k.ics, k.coff, k.clo, k.chi);
        }
        const int cx = x0 >> 1, cy = L == LAY_422 ? y0 + cr_ : y0 >> 1;
        S *du = up + (long long)cy * cw + cx, *dv = vpl + (long long)cy * cw + cx;
        if (vec_out && cx + 1 < cw) {          // W % 4 == 0: cw even, cx even
            store2(du, qu[0], qu[1]);
            store2(dv, qv[0], qv[1]);
        } else {
            du[0] = (S)qu[0];
            dv[0] = (S)qv[0];
            if (cx + 1 < cw) {
                du[1] = (S)qu[1];
                dv[1] = (S)qv[1];
            }
        }
    }
}

// ---- shutter: frames summed into an accumulator, coded or in linear light -------------------------------------------------------------
// one row of ssm_amd.video.light_curve (include/ssm_hip.h: SSM_LIGHT_ROW floats)
struct LightRow {
    float thr, islope, a, i1a, g;          // decode: c <= thr ? c * islope : ((c + a) * i1a) ^ g
    float lthr, slope, a1, ig;             // encode: L <= lthr ? L * slope : a1 * L ^ ig - a
};
static_assert(sizeof(LightRow) == SSM_LIGHT_ROW * sizeof(float), "curve row");

// x ^ e for x >= 0 as 2 ^ (e log2 x): v_log_f32, v_mul_f32, v_exp_f32, each 1 ulp by the ISA manual.  x = 0 gives log2 = -inf and 2 ^ -inf = 0.
__device__ __forceinline__ float pow_fast(float x, float e) { return __builtin_amdgcn_exp2f(e * __builtin_amdgcn_logf(x)); }

// black = (0 - mean) / sd as the ingest kernels round it.  fp32 (black * sd + mean) need not be 0 (the config's G plane gives 2^-25), so a
// value at or below black is taken as c = 0 by comparison: black stays exactly black, and sd > 0 makes the comparison the clamp's own.
__device__ __forceinline__ float light_decode(float v, float sd, float mean, float black, const LightRow &k) {
    const float c = v <= black ? 0.0f : clampf(v * sd + mean, 0.0f, 1.0f);          // the egress kernel's denormalise, clamped
    const float p = pow_fast((c + k.a) * k.i1a, k.g);
    return c <= k.thr ? c * k.islope : p;
}

__device__ __forceinline__ float light_encode(float l, float sd, float mean, const LightRow &k) {
    const float p = k.a1 * pow_fast(l, k.ig) - k.a;
    const float c = l <= k.lthr ? l * k.slope : p;              // l = 0: c = 0, and (0 - mean) / sd is the ingest kernel's black
    return (c - mean) / sd;
}

// ---- HDR transfer functions as the shutter's light: BT.2100 PQ and HLG (include/ssm_hip.h: SSM_HDR_ROW floats per kind) ------------------
// Each step below is one rounded fp32 operation; x ^ e is pow_fast, a quotient n / d is n * v_rcp_f32(d) (d stays in [0.16, 20]), the
// square root v_sqrt_f32, exp and ln are v_exp_f32 and v_log_f32 with log2 e and ln 2 folded into the row's constants on the host.
struct PqRow {
    float im2, c1, c2, c3, im1;          // decode: p = c ^ im2;  L = (max(p - c1, 0) / (c2 - c3 p)) ^ im1
    float m1, m2, pad;                   // encode: y = L ^ m1;  c = ((c1 + c2 y) / (1 + c3 y)) ^ m2, and L <= 0 gives c = 0
};
struct HlgRow {
    float third, kexp, cc, b, twelfth;   // decode: c <= 1/2 ? (c c) third : (2 ^ ((c - cc) kexp) + b) twelfth,  kexp = log2(e) / a
    float aln2, pad0, pad1;              // encode: L <= twelfth ? sqrt(3 max(L, 0)) : aln2 log2(12 L - b) + cc,  aln2 = a ln 2
};
static_assert(sizeof(PqRow) == SSM_HDR_ROW * sizeof(float) && sizeof(HlgRow) == SSM_HDR_ROW * sizeof(float), "HDR row");

__device__ __forceinline__ float quot_fast(float n, float d) { return n * __builtin_amdgcn_rcpf(d); }

// c = 0 gives p = 2 ^ -inf = 0, no numerator and L = 0: black adds no light.
__device__ __forceinline__ float light_decode(float v, float sd, float mean, float black, const PqRow &k) {
    const float c = v <= black ? 0.0f : clampf(v * sd + mean, 0.0f, 1.0f);
    const float p = pow_fast(c, k.im2);
    const float n = fmaxf(p - k.c1, 0.0f);
    const float d = k.c2 - k.c3 * p;
    return pow_fast(quot_fast(n, d), k.im1);
}

// The formula at L = 0 is c1 ^ m2 = 7.3e-7, a code that decodes to no light as every code below it does: of those codes L <= 0 takes 0,
// and (0 - mean) / sd is the ingest kernels' black.
__device__ __forceinline__ float light_encode(float l, float sd, float mean, const PqRow &k) {
    const float y = pow_fast(l, k.m1);
    const float n = k.c1 + k.c2 * y;
    const float d = 1.0f + k.c3 * y;
    const float p = pow_fast(quot_fast(n, d), k.m2);
    const float c = l <= 0.0f ? 0.0f : p;
    return (c - mean) / sd;
}

__device__ __forceinline__ float light_decode(float v, float sd, float mean, float black, const HlgRow &k) {
    const float c = v <= black ? 0.0f : clampf(v * sd + mean, 0.0f, 1.0f);
    const float lo = (c * c) * k.third;
    const float e = __builtin_amdgcn_exp2f((c - k.cc) * k.kexp);
    const float hi = (e + k.b) * k.twelfth;
    return c <= 0.5f ? lo : hi;
}

__device__ __forceinline__ float light_encode(float l, float sd, float mean, const HlgRow &k) {
    const float lo = __builtin_amdgcn_sqrtf(3.0f * fmaxf(l, 0.0f));          // l = 0: c = 0
    const float hi = k.aln2 * __builtin_amdgcn_logf(12.0f * l - k.b) + k.cc;
    const float c = l <= k.twelfth ? lo : hi;
    return (c - mean) / sd;
}

// What a mode in light adds to the kernel's arguments (its channels are three); the coded mode adds nothing.  Row is the curve's row and
// picks light_decode / light_encode by its type: LightRow (Curve<true>), PqRow or HlgRow (HdrCurve).
template <typename Row> struct InLight { Norm3 nm; Row row; int encode; };
template <bool Light> struct Curve {};
template <> struct Curve<true> : InLight<LightRow> {};
template <int Kind> struct HdrCurve;
template <> struct HdrCurve<SSM_HDR_PQ> : InLight<PqRow> {};
template <> struct HdrCurve<SSM_HDR_HLG> : InLight<HlgRow> {};

// V consecutive pixels of a row as one access: 16 bytes (V = 4: W % 4 == 0 and both views 16-byte aligned) or one float
template <int V> struct alignas(4 * V) Px { float f[V]; };

// s = init ? dec(src[0]) : acc + dec(src[0]);  s = s + dec(src[n]), n = 1 .. N-1;  r = s * scale;  acc = enc(r) - one rounded fp32 operation
// per step (the file is compiled without contraction).  Coded (Cv = Curve<false>): dec and enc are the identity, the order of
// ssm_amd.video.accumulate_host, bit for bit.  In light: dec is light_decode of the channel (blockIdx.z, three of them), enc light_encode on the
// call that closes an output (cv.encode) and the identity before.  The loads of the N frames do not depend on one another and the one
// store comes last, so the unrolled loop keeps several loads in flight per lane; the accumulator is read at most once and written once.
// The arithmetic on a Px<4> stays four scalar v_add_f32 / v_mul_f32 per step only because the Makefile builds every file with
// -fno-slp-vectorize (check_isa.sh fails the build on any v_pk_*_f32): a plain hipcc -O3 of this file packs it into v_pk_add_f32 /
// v_pk_mul_f32.
// Weighted (the shutter windows of ssm_amd.video.shutter_window): p_n = w[n] * dec(src[n]) stands where dec(src[n]) stood, one more
// rounded multiply per sample and nothing else - s = init ? p_0 : acc + p_0;  s = s + p_n;  r = s * scale;  acc = enc(r).  The weights come
// by value in the kernel's arguments (Weights<true>, SSM_ACC_WEIGHTS_MAX floats: no device buffer, no copy on the pass's stream); n is
// wave-uniform, so w[n] is a scalar load from the argument segment and the multiply takes it as a scalar operand.  Weights<false> is empty
// and the unweighted instantiations are the code they were before the template parameter.
template <bool Weighted> struct Weights {};
template <> struct Weights<true> { float w[SSM_ACC_WEIGHTS_MAX]; };

template <int V, typename Cv, bool Weighted>          // pixels per lane: 4 or 1; the mode's arguments; a weight per sample
__device__ __forceinline__ void accumulate_lane(const ssm_view &src, const ssm_view &acc, int N, int H, int W, int init, float scale, const Cv &cv,
                                                const Weights<Weighted> &wt) {
    constexpr bool Light = !std::is_same_v<Cv, Curve<false>>;
    const int x = (blockIdx.x * 64 + threadIdx.x) * V, y = blockIdx.y * 4 + threadIdx.y, c = blockIdx.z;
    if (x >= W || y >= H) return;          // V = 4: W % 4 == 0, so x + 3 < W
    float mean = 0.0f, sd = 1.0f, black = 0.0f;          // Light alone reads them
    if constexpr (Light) {
        mean = c == 0 ? cv.nm.m[0] : (c == 1 ? cv.nm.m[1] : cv.nm.m[2]), sd = c == 0 ? cv.nm.s[0] : (c == 1 ? cv.nm.s[1] : cv.nm.s[2]);
        black = (0.0f / 255.0f - mean) / sd;          // the ingest kernels' expression
    }
    const auto dec = [&](float v) {
        if constexpr (Light) return light_decode(v, sd, mean, black, cv.row);
        else return v;
    };
    const auto term = [&](float v, int n) {          // sample n's summand
        if constexpr (Weighted) return wt.w[n] * dec(v);
        else return dec(v);
    };
    const float *s = src.ptr + (long long)c * src.sc + (long long)y * src.sh + x;
    float *a = acc.ptr + (long long)c * acc.sc + (long long)y * acc.sh + x;
    Px<V> v = *reinterpret_cast<const Px<V> *>(s);
#pragma unroll
    for (int i = 0; i < V; ++i) v.f[i] = term(v.f[i], 0);
    if (!init) {
        const Px<V> o = *reinterpret_cast<const Px<V> *>(a);
#pragma unroll
        for (int i = 0; i < V; ++i) v.f[i] = o.f[i] + v.f[i];
    }
#pragma unroll 4
    for (int n = 1; n < N; ++n) {
        const Px<V> f = *reinterpret_cast<const Px<V> *>(s + (long long)n * src.sb);
#pragma unroll
        for (int i = 0; i < V; ++i) v.f[i] = v.f[i] + term(f.f[i], n);
    }
#pragma unroll
    for (int i = 0; i < V; ++i) v.f[i] = v.f[i] * scale;
    if constexpr (Light)
        if (cv.encode)
#pragma unroll
            for (int i = 0; i < V; ++i) v.f[i] = light_encode(v.f[i], sd, mean, cv.row);
    *reinterpret_cast<Px<V> *>(a) = v;
}

// One skeleton, two kernels and their weighted forms: the coded sum and the power-law curves, and the HDR transfer functions (Kind: SSM_HDR_PQ or SSM_HDR_HLG).
template <int V, bool Light>
__global__ __launch_bounds__(256) void frames_accumulate_kernel(ssm_view src, ssm_view acc, int N, int H, int W, int init, float scale,
                                                                Curve<Light> cv) {
    accumulate_lane<V>(src, acc, N, H, W, init, scale, cv, Weights<false>{});
}

template <int V, int Kind>
__global__ __launch_bounds__(256) void frames_accumulate_hdr_kernel(ssm_view src, ssm_view acc, int N, int H, int W, int init, float scale,
                                                                    HdrCurve<Kind> cv) {
    accumulate_lane<V>(src, acc, N, H, W, init, scale, cv, Weights<false>{});
}

// The weighted forms of the two: the same arguments and the N <= SSM_ACC_WEIGHTS_MAX weights after them.
template <int V, bool Light>
__global__ __launch_bounds__(256) void frames_accumulate_weighted_kernel(ssm_view src, ssm_view acc, int N, int H, int W, int init, float scale,
                                                                         Curve<Light> cv, Weights<true> wt) {
    accumulate_lane<V>(src, acc, N, H, W, init, scale, cv, wt);
}

template <int V, int Kind>
__global__ __launch_bounds__(256) void frames_accumulate_hdr_weighted_kernel(ssm_view src, ssm_view acc, int N, int H, int W, int init,
                                                                             float scale, HdrCurve<Kind> cv, Weights<true> wt) {
    accumulate_lane<V>(src, acc, N, H, W, init, scale, cv, wt);
}

// ---- sums over pairs of payloads: what the kernels share -------------------------------------------------------------------------------
// A workgroup of LANES lanes takes a span of SPAN_BYTES = 16 KiB of one plane (span_sum_kernel) or row (payload_mix_kernel): a lane CHUNKS
// pieces of 16 bytes, LANES * 16 bytes apart (a wave's loads are contiguous).  The bounds that keep the 8-bit sums in 32 bits:
//   |a - b|    a workgroup's sum is at most 255 * SPAN_BYTES < 2^22, so lane sums, wave sums and the workgroup's sum fit
//   (a - b)^2  summed over four packed bytes as a.a + b.b - 2 a.b (SseLane): a lane sees 16 * CHUNKS samples, a.a + b.b <= 2 * 65025 * 64
//              < 2^24; a workgroup's sum is at most 65025 * 16384 < 2^30
constexpr int LANES = 256, CHUNKS = 4;
constexpr long long SPAN_BYTES = (long long)LANES * 16 * CHUNKS;
static_assert(255 * SPAN_BYTES < (1ll << 32), "a workgroup's sum of absolute byte differences fits 32 bits");
static_assert(2ll * 65025 * 16 * CHUNKS < (1ll << 32), "a lane's sums of 8-bit products fit 32 bits");
static_assert(65025ll * SPAN_BYTES < (1ll << 32), "a workgroup's sum of 8-bit squares fits 32 bits");

// *dst += the sum of lane_sum over the workgroup's LANES lanes: the 64 lanes of a wave by shuffles, the waves' partials through LDS, then
// ONE 64-bit vector atomic, issued by lane 0.  Integer adds commute: the total is the same in every run.  Every lane of the workgroup
// calls it (there is a barrier inside), once per kernel.
template <typename Sum>
__device__ __forceinline__ void workgroup_add(Sum s, unsigned long long *dst) {
    __shared__ Sum partial[LANES / 64];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d);
    if ((threadIdx.x & 63) == 0) partial[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        Sum t = 0;
#pragma unroll
        for (int w = 0; w < LANES / 64; ++w) t += partial[w];
        atomicAdd(dst, (unsigned long long)t);
    }
}

// The grid's x axis counts g0 workgroups of the Y plane, then g1 of U, then g1 of V, so a workgroup belongs to ONE plane and what it
// reads never leaves it: p is the plane, g the workgroup's index inside it, `first` the plane's first sample within the payload.  luma and
// chroma are the planes' sizes in samples.  (g1 = 0: every workgroup is Y's.)
struct PlaneOf {
    int p;
    unsigned g;
    long long first;
    __device__ __forceinline__ PlaneOf(unsigned block, unsigned g0, unsigned g1, long long luma, long long chroma) : p(0), g(block) {
        if (g >= g0) {
            g -= g0, p = 1;
            if (g >= g1) g -= g1, p = 2;
        }
        first = p == 0 ? 0 : luma + (p - 1) * chroma;
    }
};

// ---- the span sums: absolute differences (scene cuts) and squared differences (hold-out scoring) ---------------------------------------
// sums[planes n + p] += sum over this workgroup's span of the lane accumulator's term of (a_n[i], b_n[i]), i over the samples of plane p
// of payload n.  planes = 1 (ssm_luma_sad_fwd: the Y plane alone, g1 = 0) or 3 (ssm_plane_sse_fwd: Y, U, V).  A lane accumulator has the
// Sample it reads, the Sum it ends in, words(x, y) for 32 bits of each operand, one(x, y) for a single sample, and sum():
//   SadLane                    |a - b|: four bytes through one v_sad_u8 (the sum of the four absolute byte differences, added to the
//                              accumulator operand), a 32-bit sum
//   SseLane<unsigned char>     (a - b)^2 over four packed bytes is  a.a + b.b - 2 a.b,  three v_dot4_u32_u8 per pair of words and no
//                              unpacking: `sq` takes a.a + b.b, `ab` takes a.b, and sq - 2 ab is the sum, exact (every term is an integer
//                              and sq >= 2 ab); a 32-bit sum
//   SseLane<unsigned short>    d^2 reaches 65535^2 = 2^32 - 131071, two of them overflow 32 bits: the lane sum is 64-bit from the first
//                              add (|d| * |d| + s as one 32 x 32 + 64 multiply-add), and so is everything after it
// The 16-byte loads need both planes' starts on 16-byte boundaries - decided per (n, plane), uniform over the workgroup.  Any other plane
// (odd frame sizes make n * frame_bytes odd, odd H or W put U and V anywhere; 4:2:0 at 45 x 71 starts U at an odd byte), and the last
// piece of a plane whose size is no multiple of a piece, goes sample by sample, samples past the plane's end never loaded.
struct SadLane {
    typedef unsigned char Sample;
    typedef unsigned Sum;
    unsigned s = 0;
    __device__ __forceinline__ void words(unsigned x, unsigned y) { s = __builtin_amdgcn_sad_u8(x, y, s); }
    __device__ __forceinline__ void one(unsigned x, unsigned y) { s += x > y ? x - y : y - x; }
    __device__ __forceinline__ Sum sum() const { return s; }
};
template <typename S> struct SseLane;
template <> struct SseLane<unsigned char> {
    typedef unsigned char Sample;
    typedef unsigned Sum;
    unsigned sq = 0, ab = 0, tail = 0;
    __device__ __forceinline__ void words(unsigned x, unsigned y) {
#if __has_builtin(__builtin_amdgcn_udot4)
        sq = __builtin_amdgcn_udot4(x, x, sq, false);
        sq = __builtin_amdgcn_udot4(y, y, sq, false);
        ab = __builtin_amdgcn_udot4(x, y, ab, false);
#else
#pragma unroll
        for (int i = 0; i < 4; ++i) one((x >> (8 * i)) & 255u, (y >> (8 * i)) & 255u);
#endif
    }
    __device__ __forceinline__ void one(unsigned x, unsigned y) {
        const int d = (int)x - (int)y;
        tail += (unsigned)(d * d);
    }
    __device__ __forceinline__ Sum sum() const { return (sq - 2u * ab) + tail; }
};
template <> struct SseLane<unsigned short> {
    typedef unsigned short Sample;
    typedef unsigned long long Sum;
    unsigned long long s = 0;
    __device__ __forceinline__ void one(unsigned x, unsigned y) {
        const unsigned d = x > y ? x - y : y - x;
        s += (unsigned long long)d * d;
    }
    __device__ __forceinline__ void words(unsigned x, unsigned y) {
        one(x & 0xffffu, y & 0xffffu);
        one(x >> 16, y >> 16);
    }
    __device__ __forceinline__ Sum sum() const { return s; }
};

template <typename Lane>
__device__ __forceinline__ void lane16(Lane &acc, i32x4 x, i32x4 y) {
    acc.words((unsigned)x.x, (unsigned)y.x);
    acc.words((unsigned)x.y, (unsigned)y.y);
    acc.words((unsigned)x.z, (unsigned)y.z);
    acc.words((unsigned)x.w, (unsigned)y.w);
}

template <typename Lane>
__global__ __launch_bounds__(LANES) void span_sum_kernel(const unsigned char *a, const unsigned char *b, long long stride_a, long long stride_b,
                                                         long long luma, long long chroma, unsigned g0, unsigned g1, int planes,
                                                         unsigned long long *sums) {          // a, b may alias; luma, chroma in samples
    typedef typename Lane::Sample S;
    constexpr int V = 16 / (int)sizeof(S);                                 // samples of a piece
    constexpr long long SPAN = SPAN_BYTES / (long long)sizeof(S);          // samples of a span
    const int n = blockIdx.y;
    const PlaneOf at(blockIdx.x, g0, g1, luma, chroma);
    const long long plane = at.p == 0 ? luma : chroma;
    const S *pa = reinterpret_cast<const S *>(a + n * stride_a) + at.first, *pb = reinterpret_cast<const S *>(b + n * stride_b) + at.first;
    const bool vec = ((reinterpret_cast<size_t>(pa) | reinterpret_cast<size_t>(pb)) & 15) == 0;
    const long long base = at.g * SPAN + threadIdx.x * V;
    Lane acc;
    if (vec && (at.g + 1) * SPAN <= plane) {          // the whole span lies inside the plane: all loads first, none guarded
        i32x4 va[CHUNKS], vb[CHUNKS];
#pragma unroll
        for (int c = 0; c < CHUNKS; ++c) {
            va[c] = *reinterpret_cast<const i32x4 *>(pa + base + (long long)c * LANES * V);
            vb[c] = *reinterpret_cast<const i32x4 *>(pb + base + (long long)c * LANES * V);
        }
#pragma unroll
        for (int c = 0; c < CHUNKS; ++c) lane16(acc, va[c], vb[c]);
    } else {
#pragma unroll
        for (int c = 0; c < CHUNKS; ++c) {
            const long long o = base + (long long)c * LANES * V;
            if (o >= plane) break;
            if (vec && o + V <= plane) {
                lane16(acc, *reinterpret_cast<const i32x4 *>(pa + o), *reinterpret_cast<const i32x4 *>(pb + o));
            } else {
#pragma unroll
                for (int i = 0; i < V; ++i)
                    if (o + i < plane) acc.one(pa[o + i], pb[o + i]);
            }
        }
    }
    workgroup_add(acc.sum(), &sums[planes * n + at.p]);
}

// ---- pulldown removal: absolute differences per field -----------------------------------------------------------------------------------
// sums[2 n + p] += sum over this workgroup's pieces in rows y = p (mod 2) of |a_n[y][x] - b_n[y][x]|: the top fields' difference at 2 n, the
// bottom fields' at 2 n + 1 (ssm_field_diff_fwd; the definition is in include/ssm_hip.h).  The rows of the two fields alternate, so the
// walk is by ROWS: piece `id` of a plane is piece k = id mod pieces of row y = id / pieces, `pieces` 16-byte pieces to a row, the last one
// ragged where the row is no multiple of 16 bytes.  The workgroup shape and the lane's work are span_sum_kernel's: LANES lanes, a lane
// CHUNKS pieces, LANES pieces apart, so a wave's lanes read neighbouring pieces of a row.  One division per lane finds its first piece;
// the next one is LANES further on, which is (y + LANES / pieces, k + LANES mod pieces) with one carry (FieldWalk, from the host).
//   |a - b|   bytes: SadLane, four per v_sad_u8; words: SadWordLane, two per v_sad_u16.  A piece's sum (at most 16 * 255, or 8 * 65535
//             < 2^19) goes to the lane's sum of the row's parity; a lane sees CHUNKS pieces and a workgroup LANES * CHUNKS, at most
//             65535 * 8 * 1024 < 2^29: both lane sums, the wave sums and the workgroup's two sums fit 32 bits.
//   loads     where both planes start on 16-byte boundaries, a row is a multiple of 16 bytes and all the workgroup's pieces exist (uniform),
//             every piece is whole and aligned: all loads first, none guarded.  Otherwise per piece: one 16-byte load per operand where
//             the piece is whole and both addresses sit on 16-byte boundaries, sample by sample where not (a row's ragged end, rows that
//             start anywhere), samples past the row's end never loaded.
//   sums      workgroup_add's steps for two sums at once: shuffles, wave partials through LDS, then lanes 0 and 1 issue ONE 64-bit vector
//             atomic each, to neighbouring words.  Integer adds: the same result in every run.
static_assert(65535ll * (16 / 2) * LANES * CHUNKS < (1ll << 32), "a workgroup's sum of absolute word differences fits 32 bits");

struct SadWordLane {
    typedef unsigned short Sample;
    typedef unsigned Sum;
    unsigned s = 0;
    __device__ __forceinline__ void one(unsigned x, unsigned y) { s += x > y ? x - y : y - x; }
    __device__ __forceinline__ void words(unsigned x, unsigned y) {
#if __has_builtin(__builtin_amdgcn_sad_u16)
        s = __builtin_amdgcn_sad_u16(x, y, s);
#else
        one(x & 0xffffu, y & 0xffffu);
        one(x >> 16, y >> 16);
#endif
    }
    __device__ __forceinline__ Sum sum() const { return s; }
};

struct FieldWalk {
    unsigned rows, cols;          // of the plane, cols in samples
    unsigned pieces, total;       // 16-byte pieces of a row (the last one may be ragged); of the plane
    unsigned dy, dk;              // LANES / pieces, LANES % pieces: from a lane's piece to its next one
};

template <typename Lane>
__global__ __launch_bounds__(LANES) void field_diff_kernel(const unsigned char *a, const unsigned char *b, long long stride_a, long long stride_b,
                                                           FieldWalk g, unsigned long long *sums) {          // a, b may alias
    typedef typename Lane::Sample S;
    constexpr unsigned V = 16 / sizeof(S);
    const int n = blockIdx.y;
    const unsigned char *pa = a + n * stride_a, *pb = b + n * stride_b;
    const long long row = (long long)g.cols * (long long)sizeof(S);
    const unsigned group = blockIdx.x * (unsigned)(LANES * CHUNKS), first = group + threadIdx.x;
    unsigned y = first / g.pieces, k = first - y * g.pieces;
    const auto next = [&]() {
        y += g.dy, k += g.dk;
        if (k >= g.pieces) k -= g.pieces, ++y;
    };
    unsigned s0 = 0, s1 = 0;          // the lane's sums over rows of parity 0 and 1
    const auto add = [&](const Lane &t, unsigned parity) {
        s0 += parity ? 0u : t.sum();
        s1 += parity ? t.sum() : 0u;
    };
    const bool even = ((reinterpret_cast<size_t>(pa) | reinterpret_cast<size_t>(pb) | (size_t)row) & 15) == 0;
    if (even && group + (unsigned)(LANES * CHUNKS) <= g.total) {
        i32x4 va[CHUNKS], vb[CHUNKS];
        unsigned parity[CHUNKS];
#pragma unroll
        for (int c = 0; c < CHUNKS; ++c) {
            const long long o = (long long)y * row + 16ll * k;
            va[c] = *reinterpret_cast<const i32x4 *>(pa + o);
            vb[c] = *reinterpret_cast<const i32x4 *>(pb + o);
            parity[c] = y & 1u;
            next();
        }
#pragma unroll
        for (int c = 0; c < CHUNKS; ++c) {
            Lane t;
            lane16(t, va[c], vb[c]);
            add(t, parity[c]);
        }
    } else {
#pragma unroll
        for (int c = 0; c < CHUNKS; ++c) {
            if (y >= g.rows) break;          // pieces are counted in row order: every later one of this lane lies past the plane too
            const long long o = (long long)y * row + 16ll * k;
            const unsigned count = min(V, g.cols - k * V);
            Lane t;
            if (count == V && ((reinterpret_cast<size_t>(pa + o) | reinterpret_cast<size_t>(pb + o)) & 15) == 0) {
                lane16(t, *reinterpret_cast<const i32x4 *>(pa + o), *reinterpret_cast<const i32x4 *>(pb + o));
            } else {
                const S *sa = reinterpret_cast<const S *>(pa + o), *sb = reinterpret_cast<const S *>(pb + o);
                for (unsigned i = 0; i < count; ++i) t.one(sa[i], sb[i]);
            }
            add(t, y & 1u);
            next();
        }
    }
    __shared__ unsigned partial[2][LANES / 64];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) s0 += __shfl_xor(s0, d), s1 += __shfl_xor(s1, d);
    if ((threadIdx.x & 63) == 0) partial[0][threadIdx.x >> 6] = s0, partial[1][threadIdx.x >> 6] = s1;
    __syncthreads();
    if (threadIdx.x < 2) {
        unsigned t = 0;
#pragma unroll
        for (int w = 0; w < LANES / 64; ++w) t += partial[threadIdx.x][w];
        atomicAdd(&sums[2 * n + threadIdx.x], (unsigned long long)t);
    }
}

// ---- field order: comb sums of a frame against the frame before and the frame after ------------------------------------------------------
// sums[3 n + {0, 1, 2}] += this workgroup's share of A0, A1, D of planes (p_n, c_n, n_n) (ssm_field_order_sums_fwd; the definition is in
// include/ssm_hip.h): over rows y = 1 .. H - 2,  s = c[y-1] + c[y+1]  and  E_r[y] = sum over x of |s - 2 r[y]|  for r = p, n, c.
// The walk is by COLUMN PIECES: a lane owns one 16-byte piece k of the rows and a band of COMB_BAND rows, y0 = 1 + COMB_BAND band, and
// goes down the band with c[y-1], c[y], c[y+1] in registers: per row one new piece of c, one of p, one of n.  Unit `id` of a plane is piece
// id mod pieces of band id / pieces, so neighbouring lanes take neighbouring pieces of the same rows; a workgroup takes LANES units.
// A band reads its two neighbour rows of c again: (COMB_BAND + 2) / COMB_BAND of c, 3.25 sample_bytes per pixel in all.
//   pieces    a piece is held as eight 32-bit registers (CombPiece): sixteen bytes widened to eight PAIRS of packed 16-bit numbers (byte
//             j of a word beside byte j + 2), eight words as one number each.  s is one add per register (510 fits a packed half), 2 r
//             one shift.  Bytes: |s - 2 r| of a pair through one v_sad_u16; words: 32-bit subtract and select, s <= 131070.
//   bounds    |s - 2 r| <= 2 * 65535 = 131070 per sample.  A row of a piece adds its E_p to one of A0, A1 and its E_n to the other, so
//             each of a lane's three sums takes at most COMB_BAND rows of 8 words: 8 * 8 * 131070 < 2^23, and a workgroup's sum of LANES of
//             them 64 * 131070 * 256 = 2147450880 < 2^31: lane sums, wave sums and the workgroup's three sums fit 32 bits.
//   loads     where the three planes start on 16-byte boundaries, a row is a multiple of 16 bytes and the lane's band is whole: every
//             piece by one 16-byte load, none guarded, all of a band's 3 COMB_BAND + 2 loads free to be in flight at once.  Otherwise per
//             piece one 16-byte load where it is whole and its address sits on a 16-byte boundary, sample by sample where not (rows that
//             start anywhere, a row's ragged end); samples past the row's end are never loaded and count as 0 in s and in r alike.
//   sums      field_diff_kernel's steps for three sums: shuffles, wave partials through LDS, then lanes 0, 1, 2 issue ONE 64-bit vector
//             atomic each.  Integer adds: the same result in every run.
constexpr int COMB_BAND = 8;
static_assert(COMB_BAND % 2 == 0, "a band starts on an odd row: the parity of row y0 + j is that of j + 1");
static_assert(131070ll * (16 / 2) * COMB_BAND * LANES < (1ll << 32), "a workgroup's comb sums of full 16-bit words fit 32 bits");

struct CombWalk {
    unsigned rows, cols;          // of the plane, cols in samples
    unsigned pieces, units;       // 16-byte pieces of a row (the last one may be ragged); pieces * bands
};

template <typename S> struct CombPiece {
    unsigned u[8];
    __device__ __forceinline__ CombPiece() {}
    __device__ __forceinline__ explicit CombPiece(i32x4 v) {
        const unsigned w[4] = {(unsigned)v.x, (unsigned)v.y, (unsigned)v.z, (unsigned)v.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (sizeof(S) == 1)
                u[2 * i] = w[i] & 0x00ff00ffu, u[2 * i + 1] = (w[i] >> 8) & 0x00ff00ffu;
            else
                u[2 * i] = w[i] & 0xffffu, u[2 * i + 1] = w[i] >> 16;
        }
    }
    // s = the row above + the row below
    __device__ __forceinline__ CombPiece plus(const CombPiece &o) const {
        CombPiece s;
#pragma unroll
        for (int i = 0; i < 8; ++i) s.u[i] = u[i] + o.u[i];
        return s;
    }
    // the sum over the piece of |s - 2 r|, *this = s
    __device__ __forceinline__ unsigned comb(const CombPiece &r) const {
        unsigned e = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const unsigned twice = r.u[i] << 1;
#if __has_builtin(__builtin_amdgcn_sad_u16)
            if (sizeof(S) == 1) {
                e = __builtin_amdgcn_sad_u16(u[i], twice, e);
                continue;
            }
#else
            if (sizeof(S) == 1) {
                const unsigned a = u[i] & 0xffffu, b = twice & 0xffffu, c = u[i] >> 16, d = twice >> 16;
                e += (a > b ? a - b : b - a) + (c > d ? c - d : d - c);
                continue;
            }
#endif
            e += u[i] > twice ? u[i] - twice : twice - u[i];
        }
        return e;
    }
};

// `count` samples at `at` as the 16 bytes of a piece, the samples past them 0
template <typename S>
__device__ __forceinline__ i32x4 comb_load(const unsigned char *at, unsigned count) {
    constexpr unsigned V = 16 / sizeof(S), PER = 4 / sizeof(S);
    if ((count == V && (reinterpret_cast<size_t>(at) & 15) == 0)) return *reinterpret_cast<const i32x4 *>(at);
    const S *s = reinterpret_cast<const S *>(at);
    unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (unsigned i = 0; i < V; ++i)
        if (i < count) w[i / PER] |= (unsigned)s[i] << (8 * sizeof(S) * (i % PER));
    i32x4 v;
    v.x = (int)w[0], v.y = (int)w[1], v.z = (int)w[2], v.w = (int)w[3];
    return v;
}

// One lane's band: rows y0 .. y0 + COMB_BAND - 1 (up to rows - 2) of piece k.  a0, a1, d take the band's share of A0, A1, D.
// y0 is odd: row y0 + j is even iff j is odd.  A0 takes E_p of the even rows and E_n of the odd ones, A1 the other two.
template <typename S>
__device__ __forceinline__ void comb_row(unsigned j, const CombPiece<S> &up, const CombPiece<S> &mid, const CombPiece<S> &down, const CombPiece<S> &rp,
                                         const CombPiece<S> &rn, unsigned &a0, unsigned &a1, unsigned &d) {
    const CombPiece<S> s = up.plus(down);
    const unsigned ep = s.comb(rp), en = s.comb(rn);
    a0 += (j & 1u) ? ep : en;
    a1 += (j & 1u) ? en : ep;
    d += s.comb(mid);
}

// a whole band of whole, aligned pieces: all 3 COMB_BAND + 2 loads first, none guarded
template <typename S>
__device__ __forceinline__ void comb_band_whole(const unsigned char *pp, const unsigned char *pc, const unsigned char *pn, long long row, unsigned y0,
                                                unsigned k, unsigned &a0, unsigned &a1, unsigned &d) {
    const long long o = (long long)(y0 - 1) * row + 16ll * k;
    i32x4 vc[COMB_BAND + 2], vp[COMB_BAND], vn[COMB_BAND];
#pragma unroll
    for (int j = 0; j < COMB_BAND + 2; ++j) vc[j] = *reinterpret_cast<const i32x4 *>(pc + o + j * row);
#pragma unroll
    for (int j = 0; j < COMB_BAND; ++j) {
        vp[j] = *reinterpret_cast<const i32x4 *>(pp + o + (j + 1) * row);
        vn[j] = *reinterpret_cast<const i32x4 *>(pn + o + (j + 1) * row);
    }
    __builtin_amdgcn_sched_barrier(0);          // the scheduler otherwise sinks the loads between the sums, three or four in flight
    CombPiece<S> up(vc[0]), mid(vc[1]);
#pragma unroll
    for (int j = 0; j < COMB_BAND; ++j) {
        const CombPiece<S> down(vc[j + 2]);
        comb_row<S>((unsigned)j, up, mid, down, CombPiece<S>(vp[j]), CombPiece<S>(vn[j]), a0, a1, d);
        up = mid, mid = down;
    }
}

// any other band, row by row: its pieces may be ragged or off a 16-byte boundary, and it may end at row rows - 2
template <typename S>
__device__ __forceinline__ void comb_band_guarded(const unsigned char *pp, const unsigned char *pc, const unsigned char *pn, long long row,
                                                  unsigned y0, unsigned k, const CombWalk &g, unsigned &a0, unsigned &a1, unsigned &d) {
    constexpr unsigned V = 16 / sizeof(S);
    const unsigned count = min(V, g.cols - k * V);
    const auto piece = [&](const unsigned char *plane, unsigned y) {
        return CombPiece<S>(comb_load<S>(plane + (long long)y * row + 16ll * k, count));
    };
    CombPiece<S> up = piece(pc, y0 - 1), mid = piece(pc, y0);
#pragma unroll 1
    for (unsigned j = 0; j < (unsigned)COMB_BAND && y0 + j + 1 < g.rows; ++j) {          // the last row with a row below it is rows - 2
        const CombPiece<S> down = piece(pc, y0 + j + 1);
        comb_row<S>(j, up, mid, down, piece(pp, y0 + j), piece(pn, y0 + j), a0, a1, d);
        up = mid, mid = down;
    }
}

template <typename S>          // the sample: unsigned char, or unsigned short (all 16 bits count)
__global__ __launch_bounds__(LANES) void field_order_sums_kernel(const unsigned char *p, const unsigned char *c, const unsigned char *nx,
                                                                 long long stride_p, long long stride_c, long long stride_n, CombWalk g,
                                                                 unsigned long long *sums) {          // p, c, nx may alias
    const int n = blockIdx.y;
    const unsigned char *pp = p + n * stride_p, *pc = c + n * stride_c, *pn = nx + n * stride_n;
    const long long row = (long long)g.cols * (long long)sizeof(S);
    const unsigned id = blockIdx.x * (unsigned)LANES + threadIdx.x;
    unsigned a0 = 0, a1 = 0, d = 0;
    if (id < g.units) {
        const unsigned band = id / g.pieces, k = id - band * g.pieces, y0 = 1u + band * (unsigned)COMB_BAND;
        const bool even = ((reinterpret_cast<size_t>(pp) | reinterpret_cast<size_t>(pc) | reinterpret_cast<size_t>(pn) | (size_t)row) & 15) == 0;
        if (even && y0 + (unsigned)COMB_BAND < g.rows)          // rows y0 - 1 .. y0 + COMB_BAND all exist
            comb_band_whole<S>(pp, pc, pn, row, y0, k, a0, a1, d);
        else
            comb_band_guarded<S>(pp, pc, pn, row, y0, k, g, a0, a1, d);
    }
    __shared__ unsigned partial[3][LANES / 64];
#pragma unroll
    for (int x = 32; x > 0; x >>= 1) a0 += __shfl_xor(a0, x), a1 += __shfl_xor(a1, x), d += __shfl_xor(d, x);
    if ((threadIdx.x & 63) == 0) partial[0][threadIdx.x >> 6] = a0, partial[1][threadIdx.x >> 6] = a1, partial[2][threadIdx.x >> 6] = d;
    __syncthreads();
    if (threadIdx.x < 3) {
        unsigned t = 0;
#pragma unroll
        for (int w = 0; w < LANES / 64; ++w) t += partial[threadIdx.x][w];
        atomicAdd(&sums[3 * n + threadIdx.x], (unsigned long long)t);
    }
}

// ---- hold-out scoring: SSIM in fixed point, summed per plane ---------------------------------------------------------------------------
// The definition is in include/ssm_hip.h (x264's and ffmpeg's construction: 4 x 4 blocks, 8 x 8 windows at stride 4, integer factors, ONE
// float64 quotient per window, rounded to a multiple of 2^-32).  sums[3 n + p] += sum over this workgroup's windows of fx.
// A workgroup owns a tile of SSIM_TW x SSIM_TH windows of ONE plane of one payload and computes the SSIM_BW x SSIM_BH = (TW + 1) x (TH + 1)
// blocks they stand on; the extra block column and row are computed again by the neighbouring tile (33 x 17 / (32 x 16) - 1 < 10 % more
// loads).  The grid's x axis counts Y's tiles (row-major), then U's, then V's; a plane without a window has no tile.
//   blocks  lane (lx, ly) of 32 x 8 takes blocks (lx, ly) and (lx, ly + 8) of the tile: four rows of four samples per operand.  Bytes: one
//           32-bit word per row where every row address of both operands is 4-byte aligned (plane start and cols multiples of 4 - per
//           (n, plane), uniform), else four byte loads; s1, s2 by udot4(x, 0x01010101), ss by udot4(x, x) + udot4(y, y), s12 by udot4(x, y):
//           a block's ss is at most 16 * 2 * 65025 < 2^22.  Words: one 8-byte load per row where the addresses are 8-byte aligned, else
//           four 2-byte loads; s1, s2 <= 16 * 65535 < 2^20 in 32 bits, ss and s12 (up to 2^37) in 64 bits from the first add.
//   windows after one barrier lane (lx, ly) forms windows (lx, ly) and (lx, ly + 8) from four LDS entries each (lx < TW, wy < TH, inside
//           the plane's window grid), evaluates fx and adds it to a signed 64-bit lane sum.  A 32-lane row of the wave reads consecutive
//           entries: no bank conflict beyond the entry's own width.
// The factors are exact in int64 (below 2^45 + c) and exact as doubles; the quotient is `/` on doubles - hipcc expands it to the IEEE
// sequence (v_div_scale_f64, v_rcp_f64, v_fma_f64 ..., v_div_fmas_f64, v_div_fixup_f64), correctly rounded as numpy's - and this file is
// compiled without contraction.  f2 f3 > 0 (c1, c2 > 0 and 64 ss >= s1^2 + s2^2), |q| <= 1 up to rounding: rint(q 2^32) fits int64.
constexpr int SSIM_LANES = LANES, SSIM_BW = 32, SSIM_BH = 16, SSIM_TW = SSIM_BW - 1, SSIM_TH = SSIM_BH - 1;
static_assert(SSIM_BW * SSIM_BH == 2 * SSIM_LANES, "a lane takes two blocks, SSIM_BH / 2 block rows apart");
static_assert(16ll * 2 * 65025 < (1ll << 32) && 16ll * 65535 < (1ll << 32), "the block sums of bytes, and s1, s2 of words, fit 32 bits");
static_assert(64ll * (64ll * 2 * 65535 * 65535) < (1ll << 46), "64 ss of a window of words stays far inside int64 and exact as a double");

template <typename S> struct SsimBlock;
template <> struct SsimBlock<unsigned char> {
    unsigned s1, s2, ss, s12;
    __device__ __forceinline__ void clear() { s1 = s2 = ss = s12 = 0; }
    __device__ __forceinline__ void row(const unsigned char *pa, const unsigned char *pb, bool vec) {
        unsigned x, y;
        if (vec) {
            x = *reinterpret_cast<const unsigned *>(pa), y = *reinterpret_cast<const unsigned *>(pb);
        } else {
            x = pa[0] | (pa[1] << 8) | (pa[2] << 16) | ((unsigned)pa[3] << 24);
            y = pb[0] | (pb[1] << 8) | (pb[2] << 16) | ((unsigned)pb[3] << 24);
        }
#if __has_builtin(__builtin_amdgcn_udot4)
        s1 = __builtin_amdgcn_udot4(x, 0x01010101u, s1, false);
        s2 = __builtin_amdgcn_udot4(y, 0x01010101u, s2, false);
        ss = __builtin_amdgcn_udot4(x, x, ss, false);
        ss = __builtin_amdgcn_udot4(y, y, ss, false);
        s12 = __builtin_amdgcn_udot4(x, y, s12, false);
#else
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const unsigned u = (x >> (8 * i)) & 255u, v = (y >> (8 * i)) & 255u;
            s1 += u, s2 += v, ss += u * u + v * v, s12 += u * v;
        }
#endif
    }
};
template <> struct SsimBlock<unsigned short> {
    unsigned long long ss, s12;
    unsigned s1, s2;
    __device__ __forceinline__ void clear() { s1 = s2 = 0, ss = s12 = 0; }
    __device__ __forceinline__ void one(unsigned u, unsigned v) {
        s1 += u, s2 += v;
        ss += (unsigned long long)u * u;
        ss += (unsigned long long)v * v;
        s12 += (unsigned long long)u * v;
    }
    __device__ __forceinline__ void row(const unsigned short *pa, const unsigned short *pb, bool vec) {
        if (vec) {
            const i32x2 x = *reinterpret_cast<const i32x2 *>(pa), y = *reinterpret_cast<const i32x2 *>(pb);
            one((unsigned)x.x & 0xffffu, (unsigned)y.x & 0xffffu);
            one((unsigned)x.x >> 16, (unsigned)y.x >> 16);
            one((unsigned)x.y & 0xffffu, (unsigned)y.y & 0xffffu);
            one((unsigned)x.y >> 16, (unsigned)y.y >> 16);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) one(pa[i], pb[i]);
        }
    }
};

// fx of one window from the sums of its four blocks (header: the order of operations is the definition)
__device__ __forceinline__ long long ssim_fx(unsigned s1, unsigned s2, unsigned long long ss, unsigned long long s12, long long c1, long long c2) {
    const long long p11 = (long long)((unsigned long long)s1 * s1), p22 = (long long)((unsigned long long)s2 * s2),
                    p12 = (long long)((unsigned long long)s1 * s2);
    const long long vars = 64ll * (long long)ss - p11 - p22, covar = 64ll * (long long)s12 - p12;
    const long long f0 = 2 * p12 + c1, f1 = 2 * covar + c2, f2 = p11 + p22 + c1, f3 = vars + c2;
    const double num = (double)f0 * (double)f1, den = (double)f2 * (double)f3;
    const double q = num / den;
    return (long long)__builtin_rint(q * 4294967296.0);
}

template <typename S>          // the sample: unsigned char, or unsigned short (all 16 bits count; the depth is in c1, c2 alone)
__global__ __launch_bounds__(SSIM_LANES) void plane_ssim_kernel(const unsigned char *a, const unsigned char *b, long long stride_a, long long stride_b,
                                                                int rows0, int cols0, int rows1, int cols1, unsigned tx0, unsigned tx1,
                                                                unsigned g0, unsigned g1, long long c1, long long c2,
                                                                unsigned long long *sums) {          // a, b may alias
    __shared__ SsimBlock<S> blk[SSIM_BH][SSIM_BW];
    const int n = blockIdx.y;
    const PlaneOf at(blockIdx.x, g0, g1, (long long)rows0 * cols0, (long long)rows1 * cols1);
    const int p = at.p;
    const unsigned g = at.g;
    const int rows = p == 0 ? rows0 : rows1, cols = p == 0 ? cols0 : cols1;
    const unsigned tx = p == 0 ? tx0 : tx1;
    const S *pa = reinterpret_cast<const S *>(a + n * stride_a) + at.first, *pb = reinterpret_cast<const S *>(b + n * stride_b) + at.first;
    const int nbx = cols >> 2, nby = rows >> 2;                            // the plane's blocks; its windows are (nbx - 1) x (nby - 1)
    const int bx0 = (int)(g % tx) * SSIM_TW, by0 = (int)(g / tx) * SSIM_TH;          // the tile's first block = its first window
    constexpr size_t ALIGN = 4 * sizeof(S);                                // a block row: 4 bytes, or 8
    const bool vec = ((reinterpret_cast<size_t>(pa) | reinterpret_cast<size_t>(pb)) % ALIGN) == 0 && (cols & 3) == 0;
    const int lx = threadIdx.x & (SSIM_BW - 1), ly = threadIdx.x / SSIM_BW;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int by = ly + h * (SSIM_BH / 2);
        if (bx0 + lx < nbx && by0 + by < nby) {          // a block of the plane: its 16 samples lie inside rows x cols
            SsimBlock<S> s;
            s.clear();
            const long long o = (long long)(4 * (by0 + by)) * cols + 4 * (bx0 + lx);
#pragma unroll
            for (int r = 0; r < 4; ++r) s.row(pa + o + (long long)r * cols, pb + o + (long long)r * cols, vec);
            blk[by][lx] = s;
        }
    }
    __syncthreads();
    long long s = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int wy = ly + h * (SSIM_BH / 2);
        if (lx < SSIM_TW && wy < SSIM_TH && bx0 + lx + 1 < nbx && by0 + wy + 1 < nby) {
            const SsimBlock<S> &q00 = blk[wy][lx], &q01 = blk[wy][lx + 1], &q10 = blk[wy + 1][lx], &q11 = blk[wy + 1][lx + 1];
            s += ssim_fx(q00.s1 + q01.s1 + q10.s1 + q11.s1, q00.s2 + q01.s2 + q10.s2 + q11.s2,
                         (unsigned long long)q00.ss + q01.ss + q10.ss + q11.ss, (unsigned long long)q00.s12 + q01.s12 + q10.s12 + q11.s12, c1, c2);
        }
    }
    workgroup_add(s, &sums[3 * n + p]);          // two's complement: the wrapped unsigned adds are the signed sum
}

// ---- repeated frames: absolute differences per 8 x 8 block, their maximum and a count per plane -----------------------------------------
// The definition is in include/ssm_hip.h: block (bx, by) of a plane is its 8 x 8 samples at (8 bx, 8 by), d = the block's sum of |a - b|;
// out[6 n + 2 p] = the largest d of plane p, out[6 n + 2 p + 1] = the number of its blocks with d > lo (ssm_block_sad_fwd).
// A workgroup owns a tile of SAD_BW x SAD_BH blocks of ONE plane of one payload, a lane one block: lane (lx, ly) of 32 x 8 takes block
// (lx, ly) of the tile, so the 32 lanes of a tile row read 32 neighbouring block rows - 256 or 512 contiguous bytes of a plane row per
// operand.  The grid's x axis counts Y's tiles (row-major), then U's, then V's; a plane without a block has no tile.
//   rows    a block row is 8 samples per operand.  Bytes: one 8-byte load, two v_sad_u8; words: one 16-byte load, four v_sad_u16 - where
//           every row address of both operands is aligned to the load (plane start and cols multiples of 8 samples - per (n, plane),
//           uniform); else sample by sample.  All eight rows of both operands are loaded before the first sum.  d <= 64 * 65535 < 2^22.
//   result  the lane's (d, d > lo) - (0, 0) where the tile leaves the plane - reduced by shuffles (max and add), 2 x 4 wave partials through
//           LDS, then lane 0 issues ONE 64-bit vector atomicMax and ONE 64-bit vector atomicAdd.  Both commute: the same words in every run.
constexpr int SAD_LANES = LANES, SAD_BW = 32, SAD_BH = 8;
static_assert(SAD_BW * SAD_BH == SAD_LANES, "a lane takes one block");
static_assert(64ll * 65535 <= (1ll << 22), "a block's sum of absolute word differences is at most 2^22");

template <typename S> struct SadRow;
template <> struct SadRow<unsigned char> {
    typedef i32x2 Vec;
    typedef SadLane Lane;
    static __device__ __forceinline__ void add(Lane &acc, Vec x, Vec y) {
        acc.words((unsigned)x.x, (unsigned)y.x);
        acc.words((unsigned)x.y, (unsigned)y.y);
    }
};
template <> struct SadRow<unsigned short> {
    typedef i32x4 Vec;
    typedef SadWordLane Lane;
    static __device__ __forceinline__ void add(Lane &acc, Vec x, Vec y) { lane16(acc, x, y); }
};

template <typename S>          // the sample: unsigned char, or unsigned short (all 16 bits count)
__global__ __launch_bounds__(SAD_LANES) void block_sad_kernel(const unsigned char *a, const unsigned char *b, long long stride_a, long long stride_b,
                                                              int rows0, int cols0, int rows1, int cols1, unsigned tx0, unsigned tx1,
                                                              unsigned g0, unsigned g1, unsigned lo,
                                                              unsigned long long *out) {          // a, b may alias
    typedef typename SadRow<S>::Vec Vec;
    const int n = blockIdx.y;
    const PlaneOf at(blockIdx.x, g0, g1, (long long)rows0 * cols0, (long long)rows1 * cols1);
    const int p = at.p;
    const int rows = p == 0 ? rows0 : rows1, cols = p == 0 ? cols0 : cols1;
    const unsigned tx = p == 0 ? tx0 : tx1;
    const S *pa = reinterpret_cast<const S *>(a + n * stride_a) + at.first, *pb = reinterpret_cast<const S *>(b + n * stride_b) + at.first;
    const int bx = (int)(at.g % tx) * SAD_BW + (int)(threadIdx.x & (SAD_BW - 1)), by = (int)(at.g / tx) * SAD_BH + (int)(threadIdx.x / SAD_BW);
    constexpr size_t ALIGN = 8 * sizeof(S);                                // a block row: 8 bytes, or 16
    const bool vec = ((reinterpret_cast<size_t>(pa) | reinterpret_cast<size_t>(pb)) % ALIGN) == 0 && (cols & 7) == 0;
    unsigned d = 0, over = 0;
    if (bx < (cols >> 3) && by < (rows >> 3)) {          // a block of the plane: its 64 samples lie inside rows x cols
        const long long o = (long long)(8 * by) * cols + 8 * bx;
        typename SadRow<S>::Lane acc;
        if (vec) {
            Vec va[8], vb[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                va[r] = *reinterpret_cast<const Vec *>(pa + o + (long long)r * cols);
                vb[r] = *reinterpret_cast<const Vec *>(pb + o + (long long)r * cols);
            }
#pragma unroll
            for (int r = 0; r < 8; ++r) SadRow<S>::add(acc, va[r], vb[r]);
        } else {
            for (int r = 0; r < 8; ++r) {
                const S *ra = pa + o + (long long)r * cols, *rb = pb + o + (long long)r * cols;
#pragma unroll
                for (int i = 0; i < 8; ++i) acc.one(ra[i], rb[i]);
            }
        }
        d = acc.sum();
        over = d > lo ? 1u : 0u;
    }
    __shared__ unsigned partial[2][SAD_LANES / 64];
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) d = max(d, (unsigned)__shfl_xor(d, s)), over += __shfl_xor(over, s);
    if ((threadIdx.x & 63) == 0) partial[0][threadIdx.x >> 6] = d, partial[1][threadIdx.x >> 6] = over;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned m = 0, c = 0;
#pragma unroll
        for (int w = 0; w < SAD_LANES / 64; ++w) m = max(m, partial[0][w]), c += partial[1][w];
        atomicMax(&out[6 * n + 2 * p], (unsigned long long)m);
        atomicAdd(&out[6 * n + 2 * p + 1], (unsigned long long)c);
    }
}

// ---- blocks that do not change: the left frame's samples kept in the outputs of a pair ---------------------------------------------------
// The definition is in include/ssm_hip.h: block (bx, by) of a FRAME is the 8 x 8 luma samples at (8 bx, 8 by) with the U and V samples under
// them, d = the sum of |a - b| over all of them; where d <= lo the block's samples of a_n are stored into the T outputs of pair n, and
// counts[n] is the number of such blocks (ssm_static_paste_fwd).
// A workgroup owns a strip of PASTE_STEPS x PASTE_BLOCKS = 256 blocks of one pair, consecutive in row-major order, and takes them 32 at a
// time (one atomic per 256 blocks: the counts of a pair share ONE word, and a workgroup per 32 blocks made 450 adders queue on it at 720p);
// the 8 lanes of a block are neighbours, lane r of them takes luma row r of the block and the chroma rows that fall to it:
//   4:2:0   one row of 4 samples: row r & 3 of the 4 x 4 under the block, of U for r < 4 and of V for r >= 4
//   4:2:2   rows r of the 8 x 4 of U and of V;   4:4:4   rows r of the 8 x 8 of U and of V
//   rows    a piece (RowPiece) is 4 or 8 samples as 1, 2 or 4 32-bit words: ONE load of its size where its address sits on a boundary of
//           that size, sample by sample into the same words where not (odd widths, a payload at an odd offset) - decided per piece, in the
//           same kernel; the store likewise.  The sums are v_sad_u8 / v_sad_u16 on the words either way.  d <= 192 * 65535 < 2^24.
//   verdict the 8 lane sums by three xor shuffles, which leave d in all 8 lanes: every lane knows its block's verdict and, where it is
//           static, stores the pieces of `a` that it loaded into the T outputs.  Nothing else is written.
//   count   one flag per block (its lane 0) through workgroup_add: shuffles, LDS partials, ONE 64-bit vector atomic per workgroup.
constexpr int PASTE_BLOCKS = LANES / 8, PASTE_STEPS = 8;
static_assert(192ll * 65535 < (1ll << 24), "a block's sum of absolute word differences over Y, U and V is below 2^24");

template <typename S, int K>          // K 32-bit words of samples S, as they stand in memory
struct RowPiece {
    unsigned w[K];
    static constexpr int PER = 4 / (int)sizeof(S), BITS = 8 * (int)sizeof(S);
    static __device__ __forceinline__ bool whole(const void *p) { return (reinterpret_cast<size_t>(p) & (size_t)(4 * K - 1)) == 0; }
    __device__ __forceinline__ void load(const unsigned char *p) {
        if (whole(p)) {
            if constexpr (K == 1) {
                w[0] = *reinterpret_cast<const unsigned *>(p);
            } else if constexpr (K == 2) {
                const i32x2 v = *reinterpret_cast<const i32x2 *>(p);
                w[0] = (unsigned)v.x, w[1] = (unsigned)v.y;
            } else {
                const i32x4 v = *reinterpret_cast<const i32x4 *>(p);
                w[0] = (unsigned)v.x, w[1] = (unsigned)v.y, w[2] = (unsigned)v.z, w[3] = (unsigned)v.w;
            }
        } else {
            const S *s = reinterpret_cast<const S *>(p);
#pragma unroll
            for (int i = 0; i < K; ++i) {
                unsigned x = 0;
#pragma unroll
                for (int k = 0; k < PER; ++k) x |= (unsigned)s[PER * i + k] << (BITS * k);
                w[i] = x;
            }
        }
    }
    __device__ __forceinline__ void store(unsigned char *p) const {
        if (whole(p)) {
            if constexpr (K == 1) {
                *reinterpret_cast<unsigned *>(p) = w[0];
            } else if constexpr (K == 2) {
                i32x2 v;
                v.x = (int)w[0], v.y = (int)w[1];
                *reinterpret_cast<i32x2 *>(p) = v;
            } else {
                i32x4 v;
                v.x = (int)w[0], v.y = (int)w[1], v.z = (int)w[2], v.w = (int)w[3];
                *reinterpret_cast<i32x4 *>(p) = v;
            }
        } else {
            S *s = reinterpret_cast<S *>(p);
#pragma unroll
            for (int i = 0; i < K; ++i)
#pragma unroll
                for (int k = 0; k < PER; ++k) s[PER * i + k] = (S)(w[i] >> (BITS * k));
        }
    }
    template <typename Lane>
    __device__ __forceinline__ void sad(Lane &acc, const RowPiece &o) const {
#pragma unroll
        for (int i = 0; i < K; ++i) acc.words(w[i], o.w[i]);
    }
};

template <typename S, int L>          // the sample and the layout (LAY_*)
__global__ __launch_bounds__(LANES) void static_paste_kernel(const unsigned char *a, const unsigned char *b, long long stride_a, long long stride_b,
                                                             unsigned char *out, long long stride_out, int T, int W, int cw, long long luma,
                                                             long long chroma, unsigned nbx, unsigned blocks, unsigned lo,
                                                             unsigned long long *counts) {          // a, b may alias; luma, chroma in samples
    constexpr int SB = (int)sizeof(S);
    constexpr int CS = L == LAY_444 ? 8 : 4;                     // chroma samples under a block row
    constexpr int KY = 8 * SB / 4, KC = CS * SB / 4;             // words of a luma piece, of a chroma piece
    constexpr int NC = L == LAY_420 ? 1 : 2;                     // chroma pieces of a lane
    const int n = blockIdx.y;
    const unsigned r = threadIdx.x & 7u;
    const unsigned char *pa = a + n * stride_a, *pb = b + n * stride_b;
    unsigned kept = 0;
    for (int step = 0; step < PASTE_STEPS; ++step) {
        const unsigned blk = (blockIdx.x * (unsigned)PASTE_STEPS + step) * (unsigned)PASTE_BLOCKS + (threadIdx.x >> 3);
        const bool live = blk < blocks;          // the same in the 8 lanes of a block
        RowPiece<S, KY> ya = {}, yb = {};
        RowPiece<S, KC> ca[NC] = {}, cb[NC] = {};
        long long oy = 0, oc[NC] = {};           // byte offsets of the lane's pieces in a payload
        unsigned d = 0;
        if (live) {          // a block of the frame: its luma rows lie inside H x W, its chroma rows inside the chroma planes
            const unsigned by = blk / nbx, bx = blk - by * nbx;
            oy = ((long long)(8 * by + r) * W + 8 * bx) * SB;
            const long long crow = L == LAY_420 ? 4 * by + (r & 3u) : 8 * by + r;
#pragma unroll
            for (int i = 0; i < NC; ++i) {
                const long long plane = L == LAY_420 ? (long long)(r >> 2) : (long long)i;
                oc[i] = (luma + plane * chroma + crow * cw + (long long)(CS * bx)) * SB;
            }
            ya.load(pa + oy), yb.load(pb + oy);
#pragma unroll
            for (int i = 0; i < NC; ++i) ca[i].load(pa + oc[i]), cb[i].load(pb + oc[i]);
            typename SadRow<S>::Lane acc;
            ya.sad(acc, yb);
#pragma unroll
            for (int i = 0; i < NC; ++i) ca[i].sad(acc, cb[i]);
            d = acc.sum();
        }
#pragma unroll
        for (int s = 1; s < 8; s <<= 1) d += __shfl_xor(d, s);          // the block's d, in its 8 lanes
        const bool keep = live && d <= lo;
        if (keep) {
            for (int j = 0; j < T; ++j) {
                unsigned char *po = out + ((long long)n * T + j) * stride_out;
                ya.store(po + oy);
#pragma unroll
                for (int i = 0; i < NC; ++i) ca[i].store(po + oc[i]);
            }
        }
        kept += keep && r == 0 ? 1u : 0u;
    }
    workgroup_add(kept, &counts[n]);
}

// ---- the flow check's per-block fallback: the nearer frame's samples where a pair's two flows contradict each other ----------------------
// The definition is in include/ssm_hip.h: the blocks are static_paste_kernel's; n(block) = the number of its 64 luma positions at which bit
// 0 of mask[0] | mask[1] is set (ssm_flow_consistency_fwd's bytes: inconsistent in at least one direction); where n > K the block's samples
// of a_n are stored into the outputs j < split of pair n and those of b_n into the outputs j >= split, and counts[n] is the number of such
// blocks (ssm_flow_paste_fwd).  The skeleton is the sibling's: strips of PASTE_STEPS x PASTE_BLOCKS blocks, 8 neighbouring lanes a block.
//   measure lane r takes the 8 mask bytes of luma row r of each direction as a RowPiece of bytes - ONE 8-byte load where the address sits on
//           an 8-byte boundary (W a multiple of 8 and an aligned plane), byte by byte where not, per piece - ORs the two, keeps bit 0 of every
//           byte and pop-counts the two words; three xor shuffles leave n <= 64 in all 8 lanes.
//   paste   where n > K every lane loads its pieces of the side's payload - a if split > 0, then b if split < T, one side after the other
//           through the same registers - and stores them into that side's outputs, by RowPiece's rule.  Nothing else is written.
//   count   one flag per block (its lane 0) through workgroup_add: ONE 64-bit vector atomic per workgroup.
// n of the block that the lane's 8 neighbours own, in all 8 of them (flow_paste_kernel, flow_mix_kernel): om is the lane's luma row in a
// mask plane, direction 1 `luma` bytes on; a lane that is not live adds nothing.  Every lane of the wave takes part in the shuffles.
__device__ __forceinline__ unsigned flow_block_bad(bool live, const unsigned char *pm, long long luma, long long om) {
    unsigned bad = 0;
    if (live) {
        RowPiece<unsigned char, 2> m0, m1;
        m0.load(pm + om), m1.load(pm + luma + om);
        bad = (unsigned)__popc((m0.w[0] | m1.w[0]) & 0x01010101u) + (unsigned)__popc((m0.w[1] | m1.w[1]) & 0x01010101u);
    }
#pragma unroll
    for (int s = 1; s < 8; s <<= 1) bad += __shfl_xor(bad, s);
    return bad;
}

template <typename S, int L>          // the sample and the layout (LAY_*)
__global__ __launch_bounds__(LANES) void flow_paste_kernel(const unsigned char *a, const unsigned char *b, long long stride_a, long long stride_b,
                                                           unsigned char *out, long long stride_out, int T, int split, int W, int cw,
                                                           long long luma, long long chroma, unsigned nbx, unsigned blocks,
                                                           const unsigned char *mask, long long stride_mask, unsigned K,
                                                           unsigned long long *counts) {          // a, b may alias; luma, chroma in samples
    constexpr int SB = (int)sizeof(S);
    constexpr int CS = L == LAY_444 ? 8 : 4;                     // chroma samples under a block row
    constexpr int KY = 8 * SB / 4, KC = CS * SB / 4;             // words of a luma piece, of a chroma piece
    constexpr int NC = L == LAY_420 ? 1 : 2;                     // chroma pieces of a lane
    const int n = blockIdx.y;
    const unsigned r = threadIdx.x & 7u;
    const unsigned char *pm = mask + n * stride_mask;            // direction 0; direction 1 is `luma` bytes on
    unsigned failed = 0;
    for (int step = 0; step < PASTE_STEPS; ++step) {
        const unsigned blk = (blockIdx.x * (unsigned)PASTE_STEPS + step) * (unsigned)PASTE_BLOCKS + (threadIdx.x >> 3);
        const bool live = blk < blocks;          // the same in the 8 lanes of a block
        long long om = 0, oy = 0, oc[NC] = {};   // the lane's luma row in a mask plane; byte offsets of its pieces in a payload
        if (live) {          // a block of the frame: its luma rows lie inside H x W, its chroma rows inside the chroma planes
            const unsigned by = blk / nbx, bx = blk - by * nbx;
            om = (long long)(8 * by + r) * W + 8 * bx;
            oy = om * SB;
            const long long crow = L == LAY_420 ? 4 * by + (r & 3u) : 8 * by + r;
#pragma unroll
            for (int i = 0; i < NC; ++i) {
                const long long plane = L == LAY_420 ? (long long)(r >> 2) : (long long)i;
                oc[i] = (luma + plane * chroma + crow * cw + (long long)(CS * bx)) * SB;
            }
        }
        const unsigned bad = flow_block_bad(live, pm, luma, om);          // the block's n, in its 8 lanes
        const bool fail = live && bad > K;
        if (fail) {
            for (int side = 0; side < 2; ++side) {
                const int j0 = side == 0 ? 0 : split, j1 = side == 0 ? split : T;
                if (j0 >= j1) continue;
                const unsigned char *ps = side == 0 ? a + n * stride_a : b + n * stride_b;
                RowPiece<S, KY> y;
                RowPiece<S, KC> c[NC];
                y.load(ps + oy);
#pragma unroll
                for (int i = 0; i < NC; ++i) c[i].load(ps + oc[i]);
                for (int j = j0; j < j1; ++j) {
                    unsigned char *po = out + ((long long)n * T + j) * stride_out;
                    y.store(po + oy);
#pragma unroll
                    for (int i = 0; i < NC; ++i) c[i].store(po + oc[i]);
                }
            }
        }
        failed += fail && r == 0 ? 1u : 0u;
    }
    workgroup_add(failed, &counts[n]);
}

// ---- hold-out scoring: the cross-fade of two payloads ---------------------------------------------------------------------------------
// out_n[i] = (a_n[i] (den - k) + b_n[i] k + (den >> 1)) / den with k = num0 + n num_step, i over the `samples` samples of a row: the
// frame-blend baseline, rounded half up.  The numerator is below 65535 * 65535 + 32768 < 2^32.  THE DIVISION is the multiply-shift of
// Granlund and Montgomery for an invariant divisor, exact for every 32-bit numerator and every den >= 2: with l = ceil(log2 den) and
// m = floor(2^32 (2^l - den) / den) + 1 (host, MixDivisor),  t = mulhi(m, x);  x / den = (t + ((x - t) >> 1)) >> (l - 1).
// ssm_amd.video_score.mix_divisor is the same pair, and tests/test_video_ssim_cpu.py proves it over the numerators the scorer can reach.
// A workgroup takes SPAN_BYTES of a row, a lane CHUNKS pieces of 16 bytes, LANES * 16 bytes apart, as span_sum_kernel does; 16-byte loads
// and stores where the three rows start on 16-byte boundaries (per n, uniform), sample by sample otherwise and in the last piece of a row
// that is no multiple of a piece.  Nothing past `samples` is loaded or stored.
static_assert(65535ll * 65535 + 32767 < (1ll << 32), "the numerator fits 32 bits unsigned");

struct MixDivisor {
    unsigned m, shift, half;          // shift = l - 1; half = den >> 1
};

__device__ __forceinline__ unsigned mix_one(unsigned x, unsigned y, unsigned wa, unsigned wb, MixDivisor d) {
    const unsigned v = x * wa + y * wb + d.half, t = __umulhi(d.m, v);
    return (t + ((v - t) >> 1)) >> d.shift;
}

template <typename S>
__device__ __forceinline__ unsigned mix_word(unsigned x, unsigned y, unsigned wa, unsigned wb, MixDivisor d) {          // 4 bytes, or 2 words
    constexpr int B = 8 * (int)sizeof(S), C = 32 / B;
    constexpr unsigned M = sizeof(S) == 1 ? 0xffu : 0xffffu;
    unsigned o = 0;
#pragma unroll
    for (int i = 0; i < C; ++i) o |= mix_one((x >> (B * i)) & M, (y >> (B * i)) & M, wa, wb, d) << (B * i);
    return o;
}

template <typename S>
__global__ __launch_bounds__(LANES) void payload_mix_kernel(const unsigned char *a, const unsigned char *b, long long stride_a, long long stride_b,
                                                                unsigned char *out, long long stride_out, long long samples, int num0,
                                                                int num_step, int den, MixDivisor d) {
    constexpr int V = 16 / (int)sizeof(S);
    constexpr long long SPAN = SPAN_BYTES / (long long)sizeof(S);
    const int n = blockIdx.y;
    const unsigned wb = (unsigned)(num0 + n * num_step), wa = (unsigned)den - wb;
    const S *pa = reinterpret_cast<const S *>(a + n * stride_a), *pb = reinterpret_cast<const S *>(b + n * stride_b);
    S *po = reinterpret_cast<S *>(out + n * stride_out);
    const bool vec = ((reinterpret_cast<size_t>(pa) | reinterpret_cast<size_t>(pb) | reinterpret_cast<size_t>(po)) & 15) == 0;
    const long long base = (long long)blockIdx.x * SPAN + threadIdx.x * V;
#pragma unroll
    for (int c = 0; c < CHUNKS; ++c) {
        const long long o = base + (long long)c * LANES * V;
        if (o >= samples) break;
        if (vec && o + V <= samples) {
            const i32x4 x = *reinterpret_cast<const i32x4 *>(pa + o), y = *reinterpret_cast<const i32x4 *>(pb + o);
            i32x4 r;
            r.x = (int)mix_word<S>((unsigned)x.x, (unsigned)y.x, wa, wb, d);
            r.y = (int)mix_word<S>((unsigned)x.y, (unsigned)y.y, wa, wb, d);
            r.z = (int)mix_word<S>((unsigned)x.z, (unsigned)y.z, wa, wb, d);
            r.w = (int)mix_word<S>((unsigned)x.w, (unsigned)y.w, wa, wb, d);
            *reinterpret_cast<i32x4 *>(po + o) = r;
        } else {
#pragma unroll
            for (int i = 0; i < V; ++i)
                if (o + i < samples) po[o + i] = (S)mix_one(pa[o + i], pb[o + i], wa, wb, d);
        }
    }
}

// ---- the flow check's per-block fallback as a cross-fade: a (1 - t) + b t where a pair's two flows contradict each other -----------------
// The definition is in include/ssm_hip.h: blocks, n(block), the test n > K and counts[n] are flow_paste_kernel's; in output j of pair n
// every sample of a failed block becomes (a (den - k_j) + b k_j + (den >> 1)) / den with k_j = num0 + j num_step - mix_one above, the exact
// rational rounded half up, so the fraction that names t does not matter (ssm_flow_mix_fwd).  The skeleton is flow_paste_kernel's: strips
// of PASTE_STEPS x PASTE_BLOCKS blocks, 8 neighbouring lanes a block, the measure through flow_block_bad.
//   mix     where n > K every lane loads its pieces of a AND of b once; per output it forms the pieces word by word (mix_word, the weights
//           two launch scalars and j) and stores them by RowPiece's rule.  Nothing else is written.  Integer multiplies only.
//   count   one flag per block (its lane 0) through workgroup_add: ONE 64-bit vector atomic per workgroup.
template <typename S, int K>
__device__ __forceinline__ RowPiece<S, K> mix_piece(const RowPiece<S, K> &x, const RowPiece<S, K> &y, unsigned wa, unsigned wb, MixDivisor d) {
    RowPiece<S, K> o;
#pragma unroll
    for (int i = 0; i < K; ++i) o.w[i] = mix_word<S>(x.w[i], y.w[i], wa, wb, d);
    return o;
}

template <typename S, int L>          // the sample and the layout (LAY_*)
__global__ __launch_bounds__(LANES) void flow_mix_kernel(const unsigned char *a, const unsigned char *b, long long stride_a, long long stride_b,
                                                         unsigned char *out, long long stride_out, int T, int num0, int num_step, int den,
                                                         MixDivisor d, int W, int cw, long long luma, long long chroma, unsigned nbx,
                                                         unsigned blocks, const unsigned char *mask, long long stride_mask, unsigned K,
                                                         unsigned long long *counts) {          // a, b may alias; luma, chroma in samples
    constexpr int SB = (int)sizeof(S);
    constexpr int CS = L == LAY_444 ? 8 : 4;                     // chroma samples under a block row
    constexpr int KY = 8 * SB / 4, KC = CS * SB / 4;             // words of a luma piece, of a chroma piece
    constexpr int NC = L == LAY_420 ? 1 : 2;                     // chroma pieces of a lane
    const int n = blockIdx.y;
    const unsigned r = threadIdx.x & 7u;
    const unsigned char *pa = a + n * stride_a, *pb = b + n * stride_b;
    const unsigned char *pm = mask + n * stride_mask;            // direction 0; direction 1 is `luma` bytes on
    unsigned failed = 0;
    for (int step = 0; step < PASTE_STEPS; ++step) {
        const unsigned blk = (blockIdx.x * (unsigned)PASTE_STEPS + step) * (unsigned)PASTE_BLOCKS + (threadIdx.x >> 3);
        const bool live = blk < blocks;          // the same in the 8 lanes of a block
        long long om = 0, oy = 0, oc[NC] = {};   // the lane's luma row in a mask plane; byte offsets of its pieces in a payload
        if (live) {          // a block of the frame: its luma rows lie inside H x W, its chroma rows inside the chroma planes
            const unsigned by = blk / nbx, bx = blk - by * nbx;
            om = (long long)(8 * by + r) * W + 8 * bx;
            oy = om * SB;
            const long long crow = L == LAY_420 ? 4 * by + (r & 3u) : 8 * by + r;
#pragma unroll
            for (int i = 0; i < NC; ++i) {
                const long long plane = L == LAY_420 ? (long long)(r >> 2) : (long long)i;
                oc[i] = (luma + plane * chroma + crow * cw + (long long)(CS * bx)) * SB;
            }
        }
        const unsigned bad = flow_block_bad(live, pm, luma, om);          // the block's n, in its 8 lanes
        const bool fail = live && bad > K;
        if (fail) {
            RowPiece<S, KY> ya, yb;
            RowPiece<S, KC> ca[NC], cb[NC];
            ya.load(pa + oy), yb.load(pb + oy);
#pragma unroll
            for (int i = 0; i < NC; ++i) ca[i].load(pa + oc[i]), cb[i].load(pb + oc[i]);
            for (int j = 0; j < T; ++j) {
                const unsigned wb = (unsigned)(num0 + j * num_step), wa = (unsigned)den - wb;
                unsigned char *po = out + ((long long)n * T + j) * stride_out;
                mix_piece(ya, yb, wa, wb, d).store(po + oy);
#pragma unroll
                for (int i = 0; i < NC; ++i) mix_piece(ca[i], cb[i], wa, wb, d).store(po + oc[i]);
            }
        }
        failed += fail && r == 0 ? 1u : 0u;
    }
    workgroup_add(failed, &counts[n]);
}

// ---- interlaced clips: fields out of frames, frames out of fields ----------------------------------------------------------------------
// A frame of H x W weaves two fields: per plane, rows of parity 0 are the top field's and rows of parity 1 the bottom field's; a field is a
// payload of the frame's layout at H/2 x W.  Both kernels walk the FRAME's rows in pieces of 16 bytes: piece `id` of a frame counts the Y
// plane's rows x pieces per row, then U's, then V's (FieldGeom::locate), so a wave's lanes take neighbouring pieces of a row and one launch
// covers the three planes.  A lane takes CHUNKS pieces, LANES pieces apart.  A piece moves as one 16-byte load and store where it is whole and
// every address involved sits on a 16-byte boundary, sample by sample otherwise (a row's ragged end; rows that start anywhere: odd widths, a
// payload at an odd offset) - decided per piece in the same kernel.  Nothing outside a row's `cols` samples is read or written.
struct FieldGeom {
    unsigned rows[3], cols[3], pieces[3];          // of the frame's planes: rows, samples per row, 16-byte pieces per row
    unsigned start[3], total;                      // first piece of a plane; pieces of a frame
    long long off[3];                              // first sample of a plane in the frame's payload; in a field's it is off / 2
};

struct FieldPiece {
    unsigned y, count;            // the frame row; samples of the piece, V or fewer at a row's end
    long long frame, field;       // byte offsets of the piece in the frame's payload and in the payload of the field that holds row y
    long long row;                // bytes of a row of the plane
    unsigned rows;                // of the frame's plane
};

template <typename S>
__device__ __forceinline__ FieldPiece field_piece(const FieldGeom &g, unsigned id) {
    constexpr unsigned V = 16 / sizeof(S);
    const int p = id >= g.start[2] ? 2 : id >= g.start[1] ? 1 : 0;
    const unsigned local = id - g.start[p], y = local / g.pieces[p], k = local - y * g.pieces[p];
    FieldPiece f;
    f.y = y, f.rows = g.rows[p];
    f.count = min(V, g.cols[p] - k * V);
    f.row = (long long)g.cols[p] * (long long)sizeof(S);
    f.frame = (g.off[p] + (long long)y * g.cols[p]) * (long long)sizeof(S) + 16ll * k;
    f.field = ((g.off[p] >> 1) + (long long)(y >> 1) * g.cols[p]) * (long long)sizeof(S) + 16ll * k;
    return f;
}

__device__ __forceinline__ bool on16(const void *a, const void *b, const void *c) {
    return ((reinterpret_cast<size_t>(a) | reinterpret_cast<size_t>(b) | reinterpret_cast<size_t>(c)) & 15) == 0;
}

// (a + b + 1) >> 1 of four packed bytes or two packed words: (a | b) - ((a ^ b) >> 1), the shifted bits kept inside their sample
template <typename S>
__device__ __forceinline__ unsigned avg_up(unsigned a, unsigned b) {
    constexpr unsigned M = sizeof(S) == 1 ? 0x7f7f7f7fu : 0x7fff7fffu;
    return (a | b) - (((a ^ b) >> 1) & M);
}

// dst = the piece at a, or with b != a the line average of the pieces at a and b
template <typename S>
__device__ __forceinline__ void move_piece(unsigned char *dst, const unsigned char *a, const unsigned char *b, unsigned count) {
    constexpr unsigned V = 16 / sizeof(S);
    if (count == V && on16(dst, a, b)) {
        i32x4 x = *reinterpret_cast<const i32x4 *>(a);
        if (b != a) {
            const i32x4 y = *reinterpret_cast<const i32x4 *>(b);
            x.x = (int)avg_up<S>((unsigned)x.x, (unsigned)y.x), x.y = (int)avg_up<S>((unsigned)x.y, (unsigned)y.y);
            x.z = (int)avg_up<S>((unsigned)x.z, (unsigned)y.z), x.w = (int)avg_up<S>((unsigned)x.w, (unsigned)y.w);
        }
        *reinterpret_cast<i32x4 *>(dst) = x;
    } else {
        const S *sa = reinterpret_cast<const S *>(a), *sb = reinterpret_cast<const S *>(b);
        S *sd = reinterpret_cast<S *>(dst);
        for (unsigned i = 0; i < count; ++i) sd[i] = (S)(((unsigned)sa[i] + (unsigned)sb[i] + 1u) >> 1);          // b == a: the sample itself
    }
}

template <typename S>
__global__ __launch_bounds__(LANES) void fields_split_kernel(const unsigned char *frames, unsigned char *fields, long long frame_bytes, FieldGeom g) {
    const int n = blockIdx.y;
    const unsigned base = blockIdx.x * (unsigned)(LANES * CHUNKS) + threadIdx.x;
    const unsigned char *src = frames + n * frame_bytes;
    unsigned char *dst = fields + n * frame_bytes;          // the frame's two fields: top at 2 n, bottom at 2 n + 1, half a frame each
#pragma unroll
    for (int c = 0; c < CHUNKS; ++c) {
        const unsigned id = base + (unsigned)c * LANES;
        if (id >= g.total) break;
        const FieldPiece f = field_piece<S>(g, id);
        const unsigned char *a = src + f.frame;
        move_piece<S>(dst + (f.y & 1) * (frame_bytes >> 1) + f.field, a, a, f.count);
    }
}

template <typename S>
__global__ __launch_bounds__(LANES) void fields_weave_kernel(const unsigned char *kept, long long stride_kept, const unsigned char *made,
                                                                 long long stride_made, unsigned char *frames, long long stride_frames, FieldGeom g,
                                                                 int parity0, int fill) {
    const int n = blockIdx.y;
    const unsigned own = (unsigned)(parity0 + n) & 1u;
    const unsigned base = blockIdx.x * (unsigned)(LANES * CHUNKS) + threadIdx.x;
    const unsigned char *pk = kept + n * stride_kept, *pm = fill ? pk : made + n * stride_made;
    unsigned char *dst = frames + n * stride_frames;
#pragma unroll
    for (int c = 0; c < CHUNKS; ++c) {
        const unsigned id = base + (unsigned)c * LANES;
        if (id >= g.total) break;
        const FieldPiece f = field_piece<S>(g, id);
        const unsigned char *a, *b;
        if ((f.y & 1u) == own) {
            a = b = pk + f.field;
        } else if (!fill) {
            a = b = pm + f.field;
        } else {
            // kept rows y - 1 and y + 1 of the frame are rows (y - 1) >> 1 and (y + 1) >> 1 of the field; f.field points at row y >> 1.
            // own = 0: y odd, the rows are y >> 1 and (y >> 1) + 1;  own = 1: y even, the rows are (y >> 1) - 1 and y >> 1.
            const long long up = own ? -f.row : 0, down = own ? 0 : f.row;
            const bool has_up = f.y >= 1, has_down = f.y + 1 < f.rows;          // a plane has at least two rows: one of them holds
            a = pk + f.field + (has_up ? up : down);
            b = pk + f.field + (has_down ? down : up);
        }
        move_piece<S>(dst + f.frame, a, b, f.count);
    }
}

// ---- letterboxed clips: luma samples above a limit per row and per column, and the cut of a window ---------------------------------------
// The definition is in include/ssm_hip.h.  rows[n H + y] += the samples of luma row y of frame n above `limit`, cols[n W + x] += those of
// column x (ssm_luma_counts_fwd; the entry clears both arrays ahead of the kernel).  A workgroup of LANES lanes owns COUNT_COLS = 256
// columns x COUNT_BAND = 32 rows of ONE frame: a lane four neighbouring columns (one 4- or 8-byte load where the plane's start and the row
// pitch are multiples of it - per n, uniform - and the four lie inside the row; sample by sample otherwise, nothing past the row's end
// loaded), wave v of the four the rows v, v + 4, ... of the band, so a wave's load is 256 or 512 contiguous bytes of a row.
//   rows   the lane's four flags summed, the wave's 64 sums by shuffles, then lane 0 issues ONE 32-bit vector atomic per row and column
//          tile (none where the sum is 0)
//   cols   four 32-bit lane counters over the wave's rows, the four waves' through LDS, then lane t issues ONE 32-bit vector atomic for
//          column t of the tile per band (none where the sum is 0)
// A count is at most H or W < 2^31.  Integer adds commute: the same words in every run.
constexpr int COUNT_COLS = 4 * 64, COUNT_BAND = 32, COUNT_WAVES = LANES / 64;
static_assert(COUNT_COLS == LANES && COUNT_BAND % COUNT_WAVES == 0, "a lane closes one column of the tile; the waves share the band's rows evenly");

template <typename S> struct Quad;          // four samples as one load
template <> struct Quad<unsigned char> {
    static __device__ __forceinline__ void load(const unsigned char *p, unsigned (&v)[4]) {
        const unsigned q = *reinterpret_cast<const unsigned *>(p);
        v[0] = q & 255u, v[1] = (q >> 8) & 255u, v[2] = (q >> 16) & 255u, v[3] = q >> 24;
    }
};
template <> struct Quad<unsigned short> {
    static __device__ __forceinline__ void load(const unsigned short *p, unsigned (&v)[4]) {
        const i32x2 q = *reinterpret_cast<const i32x2 *>(p);
        v[0] = (unsigned)q.x & 0xffffu, v[1] = (unsigned)q.x >> 16, v[2] = (unsigned)q.y & 0xffffu, v[3] = (unsigned)q.y >> 16;
    }
};

template <typename S>
__global__ __launch_bounds__(LANES) void luma_counts_kernel(const unsigned char *frames, long long stride, int H, int W, unsigned limit,
                                                            unsigned *rows, unsigned *cols) {
    __shared__ unsigned part[COUNT_WAVES][COUNT_COLS];
    const int n = blockIdx.z, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const S *plane = reinterpret_cast<const S *>(frames + n * stride);
    const long long x0 = (long long)blockIdx.x * COUNT_COLS + 4 * lane;
    const int y0 = blockIdx.y * COUNT_BAND;
    const bool vec = (reinterpret_cast<size_t>(plane) % (4 * sizeof(S))) == 0 && (W & 3) == 0;          // then x0 + 3 < W wherever x0 < W
    unsigned c[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < COUNT_BAND / COUNT_WAVES; ++k) {
        const int y = y0 + wave + k * COUNT_WAVES;
        if (y >= H) break;          // uniform over the wave
        unsigned r = 0;
        if (x0 < W) {
            const S *row = plane + (long long)y * W + x0;
            unsigned v[4] = {0u, 0u, 0u, 0u};          // 0 is above no limit
            if (vec) {
                Quad<S>::load(row, v);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (x0 + i < W) v[i] = row[i];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const unsigned f = v[i] > limit ? 1u : 0u;
                c[i] += f, r += f;
            }
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) r += __shfl_xor(r, d);
        if (lane == 0 && r) atomicAdd(&rows[(long long)n * H + y], r);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) part[wave][4 * lane + i] = c[i];
    __syncthreads();
    unsigned t = 0;
#pragma unroll
    for (int w = 0; w < COUNT_WAVES; ++w) t += part[w][threadIdx.x];
    const long long x = (long long)blockIdx.x * COUNT_COLS + threadIdx.x;
    if (x < W && t) atomicAdd(&cols[(long long)n * W + x], t);
}

// windows_n = the h x w window at (y0, x0) of frames_n, a packed payload of the same layout (ssm_window_cut_fwd): the walk of the field
// kernels over the WINDOW's rows - piece `id` counts the Y plane's rows x 16-byte pieces per row, then U's, then V's, a lane CHUNKS pieces
// LANES apart - with the source piece in the frame's plane at the plane's own origin and row pitch.  move_piece decides per piece: one
// 16-byte load and store where it is whole and both addresses sit on 16-byte boundaries, sample by sample otherwise.  Nothing outside the
// window's samples is read, nothing outside the packed window written.
struct WindowGeom {
    unsigned rows[3], cols[3], pieces[3];          // of the window's planes: rows, samples per row, 16-byte pieces per row
    unsigned start[3], total;                      // first piece of a plane; pieces of a window
    long long dst[3];                              // first sample of a plane in the window's payload
    long long src[3], pitch[3];                    // first sample of the window's part of a plane in the frame's payload; the frame plane's row
};

template <typename S>
__global__ __launch_bounds__(LANES) void window_cut_kernel(const unsigned char *frames, long long stride_in, unsigned char *windows,
                                                           long long stride_out, WindowGeom g) {
    constexpr unsigned V = 16 / sizeof(S);
    const int n = blockIdx.y;
    const unsigned base = blockIdx.x * (unsigned)(LANES * CHUNKS) + threadIdx.x;
    const unsigned char *src = frames + n * stride_in;
    unsigned char *dst = windows + n * stride_out;
#pragma unroll
    for (int c = 0; c < CHUNKS; ++c) {
        const unsigned id = base + (unsigned)c * LANES;
        if (id >= g.total) break;
        const int p = id >= g.start[2] ? 2 : id >= g.start[1] ? 1 : 0;
        const unsigned local = id - g.start[p], y = local / g.pieces[p], k = local - y * g.pieces[p];
        const unsigned count = min(V, g.cols[p] - k * V);
        const unsigned char *a = src + (g.src[p] + (long long)y * g.pitch[p]) * (long long)sizeof(S) + 16ll * k;
        move_piece<S>(dst + (g.dst[p] + (long long)y * g.cols[p]) * (long long)sizeof(S) + 16ll * k, a, a, count);
    }
}

// first and one-past-last address, in bytes, of the floats a view of [n,c,h,w] names (strides of either sign)
inline void view_range(const ssm_view &v, int n, int c, int h, int w, long long *lo, long long *hi) {
    long long a = 0, b = 0;
    const long long ext[3] = {(long long)(n - 1) * v.sb, (long long)(c - 1) * v.sc, (long long)(h - 1) * v.sh};
    for (int i = 0; i < 3; ++i) (ext[i] < 0 ? a : b) += ext[i];
    const long long base = (long long)reinterpret_cast<size_t>(v.ptr);
    *lo = base + 4 * a;
    *hi = base + 4 * (b + w);
}

inline bool view_aligned(const ssm_view &v, int floats) {
    return (reinterpret_cast<size_t>(v.ptr) % (floats * sizeof(float))) == 0 && v.sh % floats == 0 && v.sc % floats == 0 && v.sb % floats == 0;
}

inline Norm3 norm_of(const float *mean3, const float *std3) {
    Norm3 n;
    for (int c = 0; c < 3; ++c) n.m[c] = mean3[c], n.s[c] = std3[c];
    return n;
}

inline YuvRow row_of(const float *table, int matrix, int range) {
    YuvRow r;
    const float *src = table + (matrix * 2 + range) * SSM_YUV_ROW;
    float *dst = reinterpret_cast<float *>(&r);
    for (int i = 0; i < SSM_YUV_ROW; ++i) dst[i] = src[i];
    return r;
}

}  // namespace

// The planes of one frame's payload: Y is h x w, U and V ch x cw each.  The one place on the host that knows the three layouts.
struct YuvPlanes {
    int h, w, ch, cw;
    long long luma() const { return (long long)h * w; }
    long long chroma() const { return (long long)ch * cw; }
    long long frame() const { return luma() + 2 * chroma(); }          // samples of the payload
};
static YuvPlanes yuv_planes(int H, int W, int layout) {
    const bool c420 = layout == SSM_YUV_420_CENTRED || layout == SSM_YUV_420_COSITED;
    return {H, W, c420 ? (H + 1) / 2 : H, layout == SSM_YUV_444 ? W : (W + 1) / 2};
}

// The checks both pairs of entry points share; `name` is the entry point's, `what` says "chroma siting" (the 8-bit entry points, which
// take SSM_YUV_420_* and SSM_YUV_444) or "layout" (the extended ones, which take SSM_YUV_422 and the sample width as well).
static int check_yuv(const char *name, int matrix, int range, int layout, bool extended, int sample_bytes, const void *payload) {
    SSM_REQUIRE((matrix == SSM_YUV_BT601 || matrix == SSM_YUV_BT709) && (range == SSM_YUV_LIMITED || range == SSM_YUV_FULL),
                "%s: matrix %d / range %d not in {0, 1}", name, matrix, range);
    if (!extended) {
        SSM_REQUIRE(layout == SSM_YUV_420_CENTRED || layout == SSM_YUV_420_COSITED || layout == SSM_YUV_444,
                    "%s: chroma siting %d not in {0, 1, 2}", name, layout);
        return SSM_OK;
    }
    SSM_REQUIRE(layout >= SSM_YUV_420_CENTRED && layout <= SSM_YUV_422, "%s: layout %d not in {0, 1, 2, 3}", name, layout);
    SSM_REQUIRE(sample_bytes == 1 || sample_bytes == 2, "%s: sample_bytes %d not in {1, 2}", name, sample_bytes);
    SSM_REQUIRE(sample_bytes == 1 || reinterpret_cast<size_t>(payload) % 2 == 0, "%s: a payload of 2-byte samples is not 2-byte aligned", name);
    return SSM_OK;
}

// f(std::integral_constant<int, LAY_*>) of a layout: the one place where SSM_YUV_* picks a kernel instantiation
template <typename F>
static void with_layout(int layout, F f) {
    if (layout == SSM_YUV_444)
        f(std::integral_constant<int, LAY_444>{});
    else if (layout == SSM_YUV_422)
        f(std::integral_constant<int, LAY_422>{});
    else
        f(std::integral_constant<int, LAY_420>{});
}

// f(S{}) of a checked sample width, S = unsigned char or unsigned short: the one place where sample_bytes picks a kernel instantiation
template <typename F>
static void with_sample(int sample_bytes, F f) {
    if (sample_bytes == 1)
        f((unsigned char)0);
    else
        f((unsigned short)0);
}

template <typename S>
static void launch_from_yuv(const void *frames_yuv, ssm_view out, int N, int H, int W, int Hp, int Wp, int top, int left, const float *mean3,
                            const float *std3, int pad_before_norm, const float *table, int matrix, int range, int layout, void *stream) {
    const bool cos = layout != SSM_YUV_420_CENTRED;          // 4:2:2 has the co-sited case's horizontal weights (4:4:4 reads none)
    const float a0 = cos ? 0.0f : 0.25f, a1 = cos ? 1.0f : 0.75f, b1 = cos ? 0.5f : 0.75f, b2 = cos ? 0.5f : 0.25f;
    const int vec2 = (left % 2 == 0 && view_aligned(out, 2)) ? 1 : 0;
    // blocks per axis: the canvas plus the one-pixel shift of an odd offset
    const int nbx = (Wp + (left & 1) + 1) / 2, nby = (Hp + (top & 1) + 1) / 2;
    const dim3 grid((nbx + 63) / 64, (nby + 3) / 4, N);
    const long long fs = yuv_planes(H, W, layout).frame();
    const S *in = static_cast<const S *>(frames_yuv);
    with_layout(layout, [&](auto lay) {
        SSM_LAUNCH(frames_from_yuv_kernel<S, lay()>, grid, dim3(64, 4), 0, (hipStream_t)stream, in, out, H, W, Hp, Wp, top, left, fs,
                   row_of(table, matrix, range), norm_of(mean3, std3), a0, a1, b1, b2, pad_before_norm ? 1 : 0, vec2);
    });
}

static int frames_from_yuv(const char *name, const char *entry, bool extended, const void *frames_yuv, ssm_view out, int N, int H, int W, int Hp,
                           int Wp, int top, int left, const float *mean3, const float *std3, int pad_before_norm, const float *table,
                           int matrix, int range, int layout, int sample_bytes, void *stream) {
    SSM_REQUIRE(frames_yuv && out.ptr && mean3 && std3 && table, "%s: null pointer", name);
    SSM_REQUIRE(N > 0 && N <= 65535 && H > 0 && W > 0 && top >= 0 && left >= 0 && Hp >= H + top && Wp >= W + left && out.sh >= Wp &&
                    (Hp + 9) / 8 <= 65535,
                "%s: bad geometry %dx%d -> %dx%d at (%d,%d), row stride %d", name, H, W, Hp, Wp, top, left, out.sh);
    if (const int e = check_yuv(name, matrix, range, layout, extended, sample_bytes, frames_yuv)) return e;
    with_sample(sample_bytes, [&](auto s) {
        launch_from_yuv<decltype(s)>(frames_yuv, out, N, H, W, Hp, Wp, top, left, mean3, std3, pad_before_norm, table, matrix, range, layout, stream);
    });
    return ssm::check_launch(entry);
}

template <typename S>
static void launch_to_yuv(ssm_view in, void *frames_yuv, int N, int H, int W, int top, int left, const float *mean3, const float *std3,
                          const float *table, int matrix, int range, int layout, void *stream) {
    const long long fs = yuv_planes(H, W, layout).frame();
    const int vec_in = (left % 4 == 0 && view_aligned(in, 4)) ? 1 : 0;
    // W % 4 == 0 and a base aligned to four samples keep every store aligned: a Y row starts at a multiple of 4 samples; the chroma rows are
    // W / 2 (even) samples and a thread's pair starts at an even one; the Y plane is H W samples (a multiple of 4), a chroma plane
    // ceil(H/2) W/2 or H W/2 (even), a frame H W + 2 chroma planes (a multiple of 4) - so every plane of every frame starts aligned too
    const int vec_out = (W % 4 == 0 && reinterpret_cast<size_t>(frames_yuv) % (4 * sizeof(S)) == 0) ? 1 : 0;
    const dim3 grid(((W + 3) / 4 + 63) / 64, ((H + 1) / 2 + 3) / 4, N);
    S *dst = static_cast<S *>(frames_yuv);
    const int cosited = (layout == SSM_YUV_420_COSITED || layout == SSM_YUV_422) ? 1 : 0;          // (the 4:2:2 and 4:4:4 kernels do not read it)
    with_layout(layout, [&](auto lay) {
        SSM_LAUNCH(frames_to_yuv_kernel<S, lay()>, grid, dim3(64, 4), 0, (hipStream_t)stream, in, dst, H, W, top, left, fs,
                   row_of(table, matrix, range), norm_of(mean3, std3), cosited, vec_in, vec_out);
    });
}

static int frames_to_yuv(const char *name, const char *entry, bool extended, ssm_view in, void *frames_yuv, int N, int H, int W, int top, int left,
                         const float *mean3, const float *std3, const float *table, int matrix, int range, int layout, int sample_bytes,
                         void *stream) {
    SSM_REQUIRE(frames_yuv && in.ptr && mean3 && std3 && table, "%s: null pointer", name);
    SSM_REQUIRE(N > 0 && N <= 65535 && H > 0 && W > 0 && top >= 0 && left >= 0 && in.sh >= W + left && (H + 7) / 8 <= 65535,
                "%s: bad geometry %dx%d at (%d,%d), row stride %d", name, H, W, top, left, in.sh);
    if (const int e = check_yuv(name, matrix, range, layout, extended, sample_bytes, frames_yuv)) return e;
    with_sample(sample_bytes, [&](auto s) {
        launch_to_yuv<decltype(s)>(in, frames_yuv, N, H, W, top, left, mean3, std3, table, matrix, range, layout, stream);
    });
    return ssm::check_launch(entry);
}

// The 8-bit entry points are the extended ones at sample_bytes = 1, with SSM_YUV_422 refused as it always was.
extern "C" int ssm_frames_from_yuv_fwd(const unsigned char *frames_yuv, ssm_view out, int N, int H, int W, int Hp, int Wp, int top, int left,
                                       const float *mean3, const float *std3, int pad_before_norm, const float *table, int matrix,
                                       int range, int siting, void *stream) {
    return frames_from_yuv("frames_from_yuv", "ssm_frames_from_yuv_fwd", false, frames_yuv, out, N, H, W, Hp, Wp, top, left, mean3, std3,
                           pad_before_norm, table, matrix, range, siting, 1, stream);
}

extern "C" int ssm_frames_from_yuvx_fwd(const void *frames_yuv, ssm_view out, int N, int H, int W, int Hp, int Wp, int top, int left,
                                        const float *mean3, const float *std3, int pad_before_norm, const float *table, int matrix,
                                        int range, int layout, int sample_bytes, void *stream) {
    return frames_from_yuv("frames_from_yuvx", "ssm_frames_from_yuvx_fwd", true, frames_yuv, out, N, H, W, Hp, Wp, top, left, mean3, std3,
                           pad_before_norm, table, matrix, range, layout, sample_bytes, stream);
}

extern "C" int ssm_frames_to_yuv_fwd(ssm_view in, unsigned char *frames_yuv, int N, int H, int W, int top, int left, const float *mean3,
                                     const float *std3, const float *table, int matrix, int range, int siting, void *stream) {
    return frames_to_yuv("frames_to_yuv", "ssm_frames_to_yuv_fwd", false, in, frames_yuv, N, H, W, top, left, mean3, std3, table, matrix, range,
                         siting, 1, stream);
}

extern "C" int ssm_frames_to_yuvx_fwd(ssm_view in, void *frames_yuv, int N, int H, int W, int top, int left, const float *mean3,
                                      const float *std3, const float *table, int matrix, int range, int layout, int sample_bytes, void *stream) {
    return frames_to_yuv("frames_to_yuvx", "ssm_frames_to_yuvx_fwd", true, in, frames_yuv, N, H, W, top, left, mean3, std3, table, matrix, range,
                         layout, sample_bytes, stream);
}

// What the entry points in light are given beside the coded one's arguments.  kind: CURVE_ROW for a row of SSM_LIGHT_ROW floats (the
// power-law curves), or what the caller of ssm_frames_accumulate_hdr_fwd gave (SSM_HDR_*: a row of SSM_HDR_ROW floats).
enum { CURVE_ROW = -1 };
struct LightIn {
    const float *mean3, *std3, *curve;
    int encode, kind;
};

// The rows' own conditions: finite constants, and the signs that keep every logarithm's and quotient's operand where the curve is defined.
static int check_curve(const char *name, const LightRow &k) {
    bool finite = true;
    for (int i = 0; i < SSM_LIGHT_ROW; ++i) finite = finite && std::isfinite(reinterpret_cast<const float *>(&k)[i]);
    SSM_REQUIRE(finite && k.g > 0.0f && k.ig > 0.0f && k.slope > 0.0f && k.islope > 0.0f,
                "%s: curve row with g=%g (1/g=%g), slope=%g (1/slope=%g): need finite constants, g > 0 and slope > 0", name, (double)k.g,
                (double)k.ig, (double)k.slope, (double)k.islope);
    return SSM_OK;
}
static bool finite_row(const void *row) {
    bool finite = true;
    for (int i = 0; i < SSM_HDR_ROW; ++i) finite = finite && std::isfinite(static_cast<const float *>(row)[i]);
    return finite;
}
static int check_curve(const char *name, const PqRow &k) {
    SSM_REQUIRE(finite_row(&k) && k.m1 > 0.0f && k.im1 > 0.0f && k.m2 > 0.0f && k.im2 > 0.0f && k.c1 >= 0.0f && k.c3 >= 0.0f && k.c2 > k.c3,
                "%s: pq row with m1=%g (1/m1=%g), m2=%g (1/m2=%g), c1=%g, c2=%g, c3=%g: need finite constants, exponents > 0, c1 >= 0 and "
                "c2 > c3 >= 0", name, (double)k.m1, (double)k.im1, (double)k.m2, (double)k.im2, (double)k.c1, (double)k.c2, (double)k.c3);
    return SSM_OK;
}
static int check_curve(const char *name, const HlgRow &k) {
    SSM_REQUIRE(finite_row(&k) && k.third > 0.0f && k.kexp > 0.0f && k.twelfth > 0.0f && k.aln2 > 0.0f,
                "%s: hlg row with 1/3=%g, log2(e)/a=%g, 1/12=%g, a ln 2=%g: need finite constants and these four > 0", name, (double)k.third,
                (double)k.kexp, (double)k.twelfth, (double)k.aln2);
    return SSM_OK;
}

// What a weighted entry point is given beside its unweighted sibling's arguments: N host floats.
struct WeightsIn {
    const float *w;
};

// The checks and the launch of the six accumulate entry points, in one order; `light` null: the coded sum over C channels; `weighted` null:
// no weights, the kernels and the launches as they were before there were any.
static int frames_accumulate(const char *name, const char *entry, ssm_view src, ssm_view acc, int N, int C, int H, int W, int init, float scale,
                             const LightIn *light, const WeightsIn *weighted, void *stream) {
    SSM_REQUIRE(src.ptr && acc.ptr && (!light || (light->mean3 && light->std3 && light->curve)) && (!weighted || weighted->w),
                "%s: null pointer", name);
    const bool sizes = N > 0 && N <= 65535 && C > 0 && C <= 65535 && H > 0 && W > 0 && (H + 3) / 4 <= 65535;
    if (light)
        SSM_REQUIRE(sizes, "%s: bad sizes N=%d H=%d W=%d", name, N, H, W);
    else
        SSM_REQUIRE(sizes, "%s: bad sizes N=%d C=%d H=%d W=%d", name, N, C, H, W);
    Weights<true> wt = {};
    if (weighted) {
        SSM_REQUIRE(N <= SSM_ACC_WEIGHTS_MAX, "%s: N=%d frames in one weighted call: at most SSM_ACC_WEIGHTS_MAX = %d (issue the sum in pieces)",
                    name, N, SSM_ACC_WEIGHTS_MAX);
        for (int n = 0; n < N; ++n) {
            SSM_REQUIRE(std::isfinite(weighted->w[n]), "%s: weight %d must be finite (got %g)", name, n, (double)weighted->w[n]);
            wt.w[n] = weighted->w[n];
        }
    }
    SSM_REQUIRE(src.sh >= W && acc.sh >= W, "%s: row strides %d (src), %d (acc) shorter than W=%d", name, src.sh, acc.sh, W);
    SSM_REQUIRE(init == 0 || init == 1, "%s: init must be 0 or 1 (got %d)", name, init);
    if (light) SSM_REQUIRE(light->encode == 0 || light->encode == 1, "%s: encode must be 0 or 1 (got %d)", name, light->encode);
    SSM_REQUIRE(std::isfinite(scale), "%s: scale must be finite (got %g)", name, (double)scale);
    const int kind = light ? light->kind : CURVE_ROW;
    SSM_REQUIRE(kind == CURVE_ROW || kind == SSM_HDR_PQ || kind == SSM_HDR_HLG, "%s: kind %d not in {0 (pq), 1 (hlg)}", name, kind);
    Curve<true> cv;
    HdrCurve<SSM_HDR_PQ> pq;
    HdrCurve<SSM_HDR_HLG> hlg;
    if (light) {
        const float *mean3 = light->mean3, *std3 = light->std3;
        for (int c = 0; c < 3; ++c)
            SSM_REQUIRE(std::isfinite(mean3[c]) && std::isfinite(std3[c]) && std3[c] > 0.0f,
                        "%s: mean %g / std %g of channel %d: need finite values and a std above 0", name, (double)mean3[c], (double)std3[c], c);
        const auto fill = [&](auto &to, int floats) {          // the mode's arguments from the caller's; then the row's own conditions
            to.nm = norm_of(mean3, std3), to.encode = light->encode;
            for (int i = 0; i < floats; ++i) reinterpret_cast<float *>(&to.row)[i] = light->curve[i];
            return check_curve(name, to.row);
        };
        if (const int e = kind == CURVE_ROW ? fill(cv, SSM_LIGHT_ROW) : (kind == SSM_HDR_PQ ? fill(pq, SSM_HDR_ROW) : fill(hlg, SSM_HDR_ROW)))
            return e;
    }
    long long s0, s1, a0, a1;
    view_range(src, N, C, H, W, &s0, &s1);
    view_range(acc, 1, C, H, W, &a0, &a1);
    SSM_REQUIRE(s1 <= a0 || a1 <= s0, "%s: src and acc overlap (%lld bytes apart)", name, a0 - s0);
    const bool vec = W % 4 == 0 && view_aligned(src, 4) && view_aligned(acc, 4);
    const dim3 grid(((vec ? W / 4 : W) + 63) / 64, (H + 3) / 4, C);
    // the kernel at four pixels and at one pixel per lane, unweighted (k4, k1) and weighted (w4, w1), and its mode's arguments
    const auto go = [&](auto k4, auto k1, auto w4, auto w1, auto mode) {
        if (weighted)
            SSM_LAUNCH(vec ? w4 : w1, grid, dim3(64, 4), 0, (hipStream_t)stream, src, acc, N, H, W, init, scale, mode, wt);
        else
            SSM_LAUNCH(vec ? k4 : k1, grid, dim3(64, 4), 0, (hipStream_t)stream, src, acc, N, H, W, init, scale, mode);
    };
    if (!light)
        go(frames_accumulate_kernel<4, false>, frames_accumulate_kernel<1, false>, frames_accumulate_weighted_kernel<4, false>,
           frames_accumulate_weighted_kernel<1, false>, Curve<false>{});
    else if (kind == CURVE_ROW)
        go(frames_accumulate_kernel<4, true>, frames_accumulate_kernel<1, true>, frames_accumulate_weighted_kernel<4, true>,
           frames_accumulate_weighted_kernel<1, true>, cv);
    else if (kind == SSM_HDR_PQ)
        go(frames_accumulate_hdr_kernel<4, SSM_HDR_PQ>, frames_accumulate_hdr_kernel<1, SSM_HDR_PQ>,
           frames_accumulate_hdr_weighted_kernel<4, SSM_HDR_PQ>, frames_accumulate_hdr_weighted_kernel<1, SSM_HDR_PQ>, pq);
    else
        go(frames_accumulate_hdr_kernel<4, SSM_HDR_HLG>, frames_accumulate_hdr_kernel<1, SSM_HDR_HLG>,
           frames_accumulate_hdr_weighted_kernel<4, SSM_HDR_HLG>, frames_accumulate_hdr_weighted_kernel<1, SSM_HDR_HLG>, hlg);
    return ssm::check_launch(entry);
}

extern "C" int ssm_frames_accumulate_fwd(ssm_view src, ssm_view acc, int N, int C, int H, int W, int init, float scale, void *stream) {
    return frames_accumulate("frames_accumulate", "ssm_frames_accumulate_fwd", src, acc, N, C, H, W, init, scale, nullptr, nullptr, stream);
}

extern "C" int ssm_frames_accumulate_light_fwd(ssm_view src, ssm_view acc, int N, int H, int W, int init, float scale, const float *mean3,
                                               const float *std3, const float *curve, int encode, void *stream) {
    const LightIn light = {mean3, std3, curve, encode, CURVE_ROW};
    return frames_accumulate("frames_accumulate_light", "ssm_frames_accumulate_light_fwd", src, acc, N, 3, H, W, init, scale, &light, nullptr,
                             stream);
}

extern "C" int ssm_frames_accumulate_hdr_fwd(ssm_view src, ssm_view acc, int N, int H, int W, int init, float scale, const float *mean3,
                                             const float *std3, int kind, const float *consts, int encode, void *stream) {
    const LightIn light = {mean3, std3, consts, encode, kind};
    SSM_REQUIRE(kind != CURVE_ROW, "frames_accumulate_hdr: kind %d not in {0 (pq), 1 (hlg)}", kind);
    return frames_accumulate("frames_accumulate_hdr", "ssm_frames_accumulate_hdr_fwd", src, acc, N, 3, H, W, init, scale, &light, nullptr, stream);
}

// The weighted siblings: the same arguments with `weights` (host memory, N floats) after `scale`, through the same checks and launch.
extern "C" int ssm_frames_accumulate_weighted_fwd(ssm_view src, ssm_view acc, int N, int C, int H, int W, int init, float scale,
                                                  const float *weights, void *stream) {
    const WeightsIn wt = {weights};
    return frames_accumulate("frames_accumulate_weighted", "ssm_frames_accumulate_weighted_fwd", src, acc, N, C, H, W, init, scale, nullptr, &wt,
                             stream);
}

extern "C" int ssm_frames_accumulate_light_weighted_fwd(ssm_view src, ssm_view acc, int N, int H, int W, int init, float scale,
                                                        const float *weights, const float *mean3, const float *std3, const float *curve,
                                                        int encode, void *stream) {
    const LightIn light = {mean3, std3, curve, encode, CURVE_ROW};
    const WeightsIn wt = {weights};
    return frames_accumulate("frames_accumulate_light_weighted", "ssm_frames_accumulate_light_weighted_fwd", src, acc, N, 3, H, W, init, scale,
                             &light, &wt, stream);
}

extern "C" int ssm_frames_accumulate_hdr_weighted_fwd(ssm_view src, ssm_view acc, int N, int H, int W, int init, float scale,
                                                      const float *weights, const float *mean3, const float *std3, int kind,
                                                      const float *consts, int encode, void *stream) {
    const LightIn light = {mean3, std3, consts, encode, kind};
    const WeightsIn wt = {weights};
    SSM_REQUIRE(kind != CURVE_ROW, "frames_accumulate_hdr_weighted: kind %d not in {0 (pq), 1 (hlg)}", kind);
    return frames_accumulate("frames_accumulate_hdr_weighted", "ssm_frames_accumulate_hdr_weighted_fwd", src, acc, N, 3, H, W, init, scale,
                             &light, &wt, stream);
}


// ---- the pair entry points: two payloads in, sums or a third payload out -------------------------------------------------------------
// ssm_luma_sad_fwd, ssm_field_diff_fwd, ssm_field_order_sums_fwd (three operands: check_triple), ssm_plane_sse_fwd, ssm_plane_ssim_fwd, ssm_block_sad_fwd and ssm_payload_mix_fwd refuse in one order: pair_given (pointers, N), the
// entry's own sizes, check_pair (strides, alignment), what only that entry asks, grid_fits - and only then queue anything: a refused call
// queues nothing, not even the clear.
struct PairEntry {
    const char *name, *unit;          // the entry's short name; what a stride steps over: "plane", "frame" or "row"
    long long unit_bytes;             // and its size
};

static int pair_given(const char *name, const void *a, const void *b, const void *third, int N) {          // third: `sums`, or `out`
    SSM_REQUIRE(a && b && third, "%s: null pointer", name);
    SSM_REQUIRE(N > 0 && N <= 65535, "%s: N=%d outside 1..65535", name, N);
    return SSM_OK;
}

// The operands of a pair entry point once its unit is sized: the strides of a and b, of `out`, 2-byte samples, `sums`.  zero_ok: a
// stride of 0 - one payload against N - is allowed on a and b; one_waives: with N = 1 no stride of a or b is looked at.  An entry has
// either `sums`, its N or 3 N 64-bit words, or (payload_mix) `out`, a third row per n that is written: never at stride 0, and with N = 1
// its stride names nothing.
static int check_pair(const PairEntry &k, bool zero_ok, bool one_waives, const void *a, const void *b, long long stride_a, long long stride_b,
                      int N, int sample_bytes, const void *sums, const void *out = nullptr, long long stride_out = 0) {
    const char *name = k.name;
    const auto reaches = [&](long long s, bool zero) { return (zero && s == 0) || std::llabs(s) >= k.unit_bytes; };
    const bool ab_ok = (one_waives && N == 1) || (reaches(stride_a, zero_ok) && reaches(stride_b, zero_ok));
    if (zero_ok)
        SSM_REQUIRE(ab_ok, "%s: strides %lld (a), %lld (b) neither 0 nor at least the %s's %lld bytes", name, stride_a, stride_b, k.unit, k.unit_bytes);
    else
        SSM_REQUIRE(ab_ok, "%s: strides %lld (a), %lld (b) shorter than the %s's %lld bytes", name, stride_a, stride_b, k.unit, k.unit_bytes);
    if (out) SSM_REQUIRE(N == 1 || reaches(stride_out, false), "%s: stride %lld (out) shorter than the %s's %lld bytes", name, stride_out, k.unit, k.unit_bytes);
    if (sample_bytes == 2) {
        const auto odd = [](const void *p) { return reinterpret_cast<size_t>(p) % 2 != 0; };
        SSM_REQUIRE(!odd(a) && !odd(b) && !odd(out), "%s: a %s of 2-byte samples (%s) is not 2-byte aligned", name, out ? "row" : "payload",
                    out ? "a, b or out" : "a or b");
        const bool even = stride_a % 2 == 0 && stride_b % 2 == 0 && stride_out % 2 == 0;
        if (out)
            SSM_REQUIRE(even, "%s: strides %lld (a), %lld (b), %lld (out) of 2-byte samples must be even", name, stride_a, stride_b, stride_out);
        else
            SSM_REQUIRE(even, "%s: strides %lld (a), %lld (b) of 2-byte samples must be even", name, stride_a, stride_b);
    }
    if (sums) SSM_REQUIRE(reinterpret_cast<size_t>(sums) % 8 == 0, "%s: sums is not 8-byte aligned", name);
    return SSM_OK;
}

static int grid_fits(const PairEntry &k, long long groups) {
    SSM_REQUIRE(groups <= 2147483647ll, "%s: a %s of %lld bytes is more than the grid takes", k.name, k.unit, k.unit_bytes);
    return SSM_OK;
}

// The entry's clear of its `words` 64-bit sums, on the caller's stream ahead of the kernel; called after every check.
static int clear_sums(const char *name, void *sums, size_t words, void *stream) {
    const hipError_t e = ssm::memset_async(sums, 0, sizeof(unsigned long long) * words, (hipStream_t)stream);
    if (e != hipSuccess) {
        ssm::set_error("%s: memset failed: %s", name, hipGetErrorString(e));
        return SSM_E_LAUNCH;
    }
    return SSM_OK;
}

// what the two scoring entry points check of a frame before they size it
static int check_frame(const char *name, int H, int W, int layout, int sample_bytes) {
    SSM_REQUIRE(H > 0 && W > 0, "%s: bad frame size %dx%d", name, H, W);
    SSM_REQUIRE(layout >= SSM_YUV_420_CENTRED && layout <= SSM_YUV_422, "%s: layout %d not in {0, 1, 2, 3}", name, layout);
    SSM_REQUIRE(sample_bytes == 1 || sample_bytes == 2, "%s: sample_bytes %d not in {1, 2}", name, sample_bytes);
    return SSM_OK;
}

extern "C" int ssm_luma_sad_fwd(const unsigned char *a, const unsigned char *b, long long stride_a, long long stride_b, int N, int H, int W,
                                unsigned long long *sums, void *stream) {
    if (const int e = pair_given("luma_sad", a, b, sums, N)) return e;
    SSM_REQUIRE(H > 0 && W > 0, "luma_sad: bad plane size %dx%d", H, W);
    const long long plane = (long long)H * W, groups = (plane + SPAN_BYTES - 1) / SPAN_BYTES;
    const PairEntry k = {"luma_sad", "plane", plane};
    if (const int e = check_pair(k, false, true, a, b, stride_a, stride_b, N, 1, sums)) return e;
    if (const int e = grid_fits(k, groups)) return e;
    if (const int e = clear_sums(k.name, sums, (size_t)N, stream)) return e;
    // one plane per payload: every workgroup is Y's (g1 = 0), sums[n]
    SSM_LAUNCH(span_sum_kernel<SadLane>, dim3((unsigned)groups, N), dim3(LANES), 0, (hipStream_t)stream, a, b, stride_a, stride_b, plane, 0ll,
               (unsigned)groups, 0u, 1, sums);
    return ssm::check_launch("ssm_luma_sad_fwd");
}

extern "C" int ssm_field_diff_fwd(const void *a, const void *b, long long stride_a, long long stride_b, int N, int H, int W, int sample_bytes,
                                  unsigned long long *sums, void *stream) {
    if (const int e = pair_given("field_diff", a, b, sums, N)) return e;
    SSM_REQUIRE(H > 0 && W > 0, "field_diff: bad plane size %dx%d", H, W);
    SSM_REQUIRE(sample_bytes == 1 || sample_bytes == 2, "field_diff: sample_bytes %d not in {1, 2}", sample_bytes);
    const long long row = (long long)W * sample_bytes, pieces = (row + 15) / 16, total = pieces * H;
    const PairEntry k = {"field_diff", "plane", row * H};
    if (const int e = check_pair(k, true, false, a, b, stride_a, stride_b, N, sample_bytes, sums)) return e;
    if (const int e = grid_fits(k, total)) return e;          // a piece's index, and the last workgroup's past the plane, fit 32 bits
    if (const int e = clear_sums(k.name, sums, 2 * (size_t)N, stream)) return e;
    const FieldWalk g = {(unsigned)H, (unsigned)W, (unsigned)pieces, (unsigned)total, (unsigned)(LANES / pieces), (unsigned)(LANES % pieces)};
    const long long groups = (total + LANES * CHUNKS - 1) / (LANES * CHUNKS);
    const unsigned char *pa = static_cast<const unsigned char *>(a), *pb = static_cast<const unsigned char *>(b);
    with_sample(sample_bytes, [&](auto s) {
        typedef std::conditional_t<sizeof(s) == 1, SadLane, SadWordLane> Lane;
        SSM_LAUNCH(field_diff_kernel<Lane>, dim3((unsigned)groups, N), dim3(LANES), 0, (hipStream_t)stream, pa, pb, stride_a, stride_b, g, sums);
    });
    return ssm::check_launch("ssm_field_diff_fwd");
}

// Three operands that are only read: check_pair's questions in its order and words, asked of p, c and n.
static int check_triple(const PairEntry &k, const void *p, const void *c, const void *n, long long stride_p, long long stride_c,
                        long long stride_n, int sample_bytes, const void *sums) {
    const char *name = k.name;
    const auto reaches = [&](long long s) { return s == 0 || std::llabs(s) >= k.unit_bytes; };
    SSM_REQUIRE(reaches(stride_p) && reaches(stride_c) && reaches(stride_n),
                "%s: strides %lld (p), %lld (c), %lld (n) neither 0 nor at least the %s's %lld bytes", name, stride_p, stride_c, stride_n, k.unit,
                k.unit_bytes);
    if (sample_bytes == 2) {
        const auto odd = [](const void *q) { return reinterpret_cast<size_t>(q) % 2 != 0; };
        SSM_REQUIRE(!odd(p) && !odd(c) && !odd(n), "%s: a payload of 2-byte samples (p, c or n) is not 2-byte aligned", name);
        SSM_REQUIRE(stride_p % 2 == 0 && stride_c % 2 == 0 && stride_n % 2 == 0,
                    "%s: strides %lld (p), %lld (c), %lld (n) of 2-byte samples must be even", name, stride_p, stride_c, stride_n);
    }
    SSM_REQUIRE(reinterpret_cast<size_t>(sums) % 8 == 0, "%s: sums is not 8-byte aligned", name);
    return SSM_OK;
}

extern "C" int ssm_field_order_sums_fwd(const void *p, const void *c, const void *n, long long stride_p, long long stride_c, long long stride_n,
                                        int N, int H, int W, int sample_bytes, unsigned long long *sums, void *stream) {
    SSM_REQUIRE(p, "field_order_sums: null pointer");
    if (const int e = pair_given("field_order_sums", c, n, sums, N)) return e;
    SSM_REQUIRE(H > 0 && W > 0, "field_order_sums: bad plane size %dx%d", H, W);
    SSM_REQUIRE(sample_bytes == 1 || sample_bytes == 2, "field_order_sums: sample_bytes %d not in {1, 2}", sample_bytes);
    const long long row = (long long)W * sample_bytes, pieces = (row + 15) / 16;
    const long long bands = H < 3 ? 0 : (H - 2 + COMB_BAND - 1) / COMB_BAND, units = pieces * bands;
    const PairEntry k = {"field_order_sums", "plane", row * H};
    if (const int e = check_triple(k, p, c, n, stride_p, stride_c, stride_n, sample_bytes, sums)) return e;
    if (const int e = grid_fits(k, pieces * H)) return e;          // a unit's index, and the last workgroup's past the plane, fit 32 bits
    if (const int e = clear_sums(k.name, sums, 3 * (size_t)N, stream)) return e;
    if (units == 0) return SSM_OK;          // H < 3: no row has a row above and a row below, three zeros
    const CombWalk g = {(unsigned)H, (unsigned)W, (unsigned)pieces, (unsigned)units};
    const long long groups = (units + LANES - 1) / LANES;
    const unsigned char *pp = static_cast<const unsigned char *>(p), *pc = static_cast<const unsigned char *>(c),
                        *pn = static_cast<const unsigned char *>(n);
    with_sample(sample_bytes, [&](auto s) {
        SSM_LAUNCH(field_order_sums_kernel<decltype(s)>, dim3((unsigned)groups, N), dim3(LANES), 0, (hipStream_t)stream, pp, pc, pn, stride_p,
                   stride_c, stride_n, g, sums);
    });
    return ssm::check_launch("ssm_field_order_sums_fwd");
}

extern "C" int ssm_plane_sse_fwd(const void *a, const void *b, long long stride_a, long long stride_b, int N, int H, int W, int layout,
                                 int sample_bytes, unsigned long long *sums, void *stream) {
    if (const int e = pair_given("plane_sse", a, b, sums, N)) return e;
    if (const int e = check_frame("plane_sse", H, W, layout, sample_bytes)) return e;
    const YuvPlanes pl = yuv_planes(H, W, layout);
    const PairEntry k = {"plane_sse", "frame", pl.frame() * sample_bytes};
    if (const int e = check_pair(k, true, false, a, b, stride_a, stride_b, N, sample_bytes, sums)) return e;
    const long long span = SPAN_BYTES / sample_bytes, g0 = (pl.luma() + span - 1) / span, g1 = (pl.chroma() + span - 1) / span;
    if (const int e = grid_fits(k, g0 + 2 * g1)) return e;
    if (const int e = clear_sums(k.name, sums, 3 * (size_t)N, stream)) return e;
    const unsigned char *pa = static_cast<const unsigned char *>(a), *pb = static_cast<const unsigned char *>(b);
    with_sample(sample_bytes, [&](auto s) {
        SSM_LAUNCH(span_sum_kernel<SseLane<decltype(s)>>, dim3((unsigned)(g0 + 2 * g1), N), dim3(LANES), 0, (hipStream_t)stream, pa, pb, stride_a,
                   stride_b, pl.luma(), pl.chroma(), (unsigned)g0, (unsigned)g1, 3, sums);
    });
    return ssm::check_launch("ssm_plane_sse_fwd");
}

// the windows of a plane of rows x cols samples along one axis: (samples >> 2) - 1 blocks' worth, 0 below 8 samples
static long long ssim_windows(int samples) { return (samples >> 2) > 1 ? (samples >> 2) - 1 : 0; }

extern "C" int ssm_plane_ssim_fwd(const void *a, const void *b, long long stride_a, long long stride_b, int N, int H, int W, int layout,
                                  int sample_bytes, long long c1, long long c2, long long *sums, void *stream) {
    if (const int e = pair_given("plane_ssim", a, b, sums, N)) return e;
    if (const int e = check_frame("plane_ssim", H, W, layout, sample_bytes)) return e;
    SSM_REQUIRE(c1 > 0 && c2 > 0 && c1 <= (1ll << 40) && c2 <= (1ll << 40), "plane_ssim: c1=%lld, c2=%lld outside 1..2^40", c1, c2);
    const YuvPlanes pl = yuv_planes(H, W, layout);
    const PairEntry k = {"plane_ssim", "frame", pl.frame() * sample_bytes};
    if (const int e = check_pair(k, true, false, a, b, stride_a, stride_b, N, sample_bytes, sums)) return e;
    const long long tx0 = (ssim_windows(pl.w) + SSIM_TW - 1) / SSIM_TW, ty0 = (ssim_windows(pl.h) + SSIM_TH - 1) / SSIM_TH;
    const long long tx1 = (ssim_windows(pl.cw) + SSIM_TW - 1) / SSIM_TW, ty1 = (ssim_windows(pl.ch) + SSIM_TH - 1) / SSIM_TH;
    const long long g0 = tx0 * ty0, g1 = tx1 * ty1;
    if (const int e = grid_fits(k, g0 + 2 * g1)) return e;
    if (const int e = clear_sums(k.name, sums, 3 * (size_t)N, stream)) return e;
    if (g0 + 2 * g1 == 0) return SSM_OK;          // no plane has a window: the cleared sums are the result
    const unsigned char *pa = static_cast<const unsigned char *>(a), *pb = static_cast<const unsigned char *>(b);
    with_sample(sample_bytes, [&](auto s) {
        SSM_LAUNCH(plane_ssim_kernel<decltype(s)>, dim3((unsigned)(g0 + 2 * g1), N), dim3(SSIM_LANES), 0, (hipStream_t)stream, pa, pb, stride_a,
                   stride_b, pl.h, pl.w, pl.ch, pl.cw, (unsigned)tx0, (unsigned)tx1, (unsigned)g0, (unsigned)g1, c1, c2,
                   reinterpret_cast<unsigned long long *>(sums));
    });
    return ssm::check_launch("ssm_plane_ssim_fwd");
}

extern "C" int ssm_block_sad_fwd(const void *a, const void *b, long long stride_a, long long stride_b, int N, int H, int W, int layout,
                                 int sample_bytes, int lo, unsigned long long *out, void *stream) {
    if (const int e = pair_given("block_sad", a, b, out, N)) return e;
    if (const int e = check_frame("block_sad", H, W, layout, sample_bytes)) return e;
    const YuvPlanes pl = yuv_planes(H, W, layout);
    const PairEntry k = {"block_sad", "frame", pl.frame() * sample_bytes};
    if (const int e = check_pair(k, true, false, a, b, stride_a, stride_b, N, sample_bytes, nullptr)) return e;
    SSM_REQUIRE(lo >= 0 && lo <= (1 << 22), "block_sad: lo=%d outside 0..2^22", lo);
    SSM_REQUIRE(reinterpret_cast<size_t>(out) % 8 == 0, "block_sad: out is not 8-byte aligned");
    const auto tiles = [](int samples, int per) { return (long long)((samples >> 3) + per - 1) / per; };
    const long long tx0 = tiles(pl.w, SAD_BW), tx1 = tiles(pl.cw, SAD_BW);
    const long long g0 = tx0 * tiles(pl.h, SAD_BH), g1 = tx1 * tiles(pl.ch, SAD_BH);
    if (const int e = grid_fits(k, g0 + 2 * g1)) return e;
    if (const int e = clear_sums(k.name, out, 6 * (size_t)N, stream)) return e;
    if (g0 + 2 * g1 == 0) return SSM_OK;          // no plane has a block: the cleared words are the result
    const unsigned char *pa = static_cast<const unsigned char *>(a), *pb = static_cast<const unsigned char *>(b);
    with_sample(sample_bytes, [&](auto s) {
        SSM_LAUNCH(block_sad_kernel<decltype(s)>, dim3((unsigned)(g0 + 2 * g1), N), dim3(SAD_LANES), 0, (hipStream_t)stream, pa, pb, stride_a,
                   stride_b, pl.h, pl.w, pl.ch, pl.cw, (unsigned)tx0, (unsigned)tx1, (unsigned)g0, (unsigned)g1, (unsigned)lo, out);
    });
    return ssm::check_launch("ssm_block_sad_fwd");
}

// first and one-past-last byte address of N rows of `row` bytes, `stride` bytes apart (either sign, or 0)
static void rows_range(const void *p, long long stride, long long N, long long row, long long *lo, long long *hi) {
    const long long base = (long long)reinterpret_cast<size_t>(p), ext = (N - 1) * stride;
    *lo = base + (ext < 0 ? ext : 0);
    *hi = base + (ext > 0 ? ext : 0) + row;
}

// the divisor of mix_one for den in 2..65535 (the header of payload_mix_kernel spells the construction)
static MixDivisor mix_divisor(int den) {
    int l = 0;
    while ((1ll << l) < den) ++l;          // ceil(log2 den) >= 1
    MixDivisor d;
    d.m = (unsigned)((((1ull << l) - (unsigned long long)den) << 32) / (unsigned long long)den + 1ull);
    d.shift = (unsigned)(l - 1), d.half = (unsigned)(den >> 1);
    return d;
}

extern "C" int ssm_payload_mix_fwd(const void *a, const void *b, long long stride_a, long long stride_b, void *out, long long stride_out, int N,
                                   long long samples, int sample_bytes, int num0, int num_step, int den, void *stream) {
    if (const int e = pair_given("payload_mix", a, b, out, N)) return e;
    SSM_REQUIRE(samples > 0, "payload_mix: samples=%lld must be positive", samples);
    SSM_REQUIRE(sample_bytes == 1 || sample_bytes == 2, "payload_mix: sample_bytes %d not in {1, 2}", sample_bytes);
    SSM_REQUIRE(den >= 2 && den <= 65535, "payload_mix: den=%d outside 2..65535", den);
    const long long k_last = (long long)num0 + (long long)(N - 1) * num_step;
    SSM_REQUIRE(num0 >= 0 && num0 <= den && k_last >= 0 && k_last <= den, "payload_mix: k = %d + n * %d leaves 0..den=%d within N=%d rows", num0,
                num_step, den, N);
    const long long row = samples * sample_bytes;
    const PairEntry k = {"payload_mix", "row", row};
    if (const int e = check_pair(k, true, false, a, b, stride_a, stride_b, N, sample_bytes, nullptr, out, stride_out)) return e;
    long long o0, o1, a0, a1, b0, b1;
    rows_range(out, stride_out, N, row, &o0, &o1);
    rows_range(a, stride_a, N, row, &a0, &a1);
    rows_range(b, stride_b, N, row, &b0, &b1);
    SSM_REQUIRE((a1 <= o0 || o1 <= a0) && (b1 <= o0 || o1 <= b0), "payload_mix: out overlaps a or b");
    const long long span = SPAN_BYTES / sample_bytes, groups = (samples + span - 1) / span;
    if (const int e = grid_fits(k, groups)) return e;
    const MixDivisor d = mix_divisor(den);
    const unsigned char *pa = static_cast<const unsigned char *>(a), *pb = static_cast<const unsigned char *>(b);
    with_sample(sample_bytes, [&](auto s) {
        SSM_LAUNCH(payload_mix_kernel<decltype(s)>, dim3((unsigned)groups, N), dim3(LANES), 0, (hipStream_t)stream, pa, pb, stride_a, stride_b,
                   static_cast<unsigned char *>(out), stride_out, samples, num0, num_step, den, d);
    });
    return ssm::check_launch("ssm_payload_mix_fwd");
}

// ssm_static_paste_fwd refuses in the order of its header section - pointers, N and T, the frame, lo, the strides of a and b, of out, 2-byte
// alignment, overlap, counts, the grid - and only then queues the clear and, for a frame that has blocks, the one launch.
extern "C" int ssm_static_paste_fwd(const void *a, const void *b, long long stride_a, long long stride_b, void *out, long long stride_out, int N,
                                    int T, int H, int W, int layout, int sample_bytes, unsigned int lo, unsigned long long *counts, void *stream) {
    const char *name = "static_paste";
    SSM_REQUIRE(a && b && out && counts, "%s: null pointer", name);
    SSM_REQUIRE(N > 0 && N <= 65535, "%s: N=%d outside 1..65535", name, N);
    SSM_REQUIRE(T > 0 && T <= 65535, "%s: T=%d outside 1..65535", name, T);
    if (const int e = check_frame(name, H, W, layout, sample_bytes)) return e;
    SSM_REQUIRE(lo < (1u << 24), "%s: lo=%u outside 0..2^24-1", name, lo);
    const YuvPlanes pl = yuv_planes(H, W, layout);
    const long long fb = pl.frame() * sample_bytes, outs = (long long)N * T;
    const PairEntry k = {name, "frame", fb};
    SSM_REQUIRE(N == 1 || (std::llabs(stride_a) >= fb && std::llabs(stride_b) >= fb), "%s: strides %lld (a), %lld (b) shorter than the frame's %lld bytes",
                name, stride_a, stride_b, fb);
    SSM_REQUIRE(outs == 1 || std::llabs(stride_out) >= fb, "%s: stride %lld (out) shorter than the frame's %lld bytes", name, stride_out, fb);
    if (sample_bytes == 2) {
        const auto odd = [](const void *p) { return reinterpret_cast<size_t>(p) % 2 != 0; };
        SSM_REQUIRE(!odd(a) && !odd(b) && !odd(out), "%s: a payload of 2-byte samples (a, b or out) is not 2-byte aligned", name);
        SSM_REQUIRE(stride_a % 2 == 0 && stride_b % 2 == 0 && stride_out % 2 == 0, "%s: strides %lld (a), %lld (b), %lld (out) of 2-byte samples must be even",
                    name, stride_a, stride_b, stride_out);
    }
    long long o0, o1, a0, a1, b0, b1;
    rows_range(out, stride_out, outs, fb, &o0, &o1);
    rows_range(a, stride_a, N, fb, &a0, &a1);
    rows_range(b, stride_b, N, fb, &b0, &b1);
    SSM_REQUIRE((a1 <= o0 || o1 <= a0) && (b1 <= o0 || o1 <= b0), "%s: out overlaps a or b", name);
    SSM_REQUIRE(reinterpret_cast<size_t>(counts) % 8 == 0, "%s: counts is not 8-byte aligned", name);
    const long long nbx = W >> 3, blocks = nbx * (H >> 3), strip = PASTE_BLOCKS * PASTE_STEPS, groups = (blocks + strip - 1) / strip;
    if (const int e = grid_fits(k, groups)) return e;
    if (const int e = clear_sums(name, counts, (size_t)N, stream)) return e;
    if (blocks == 0) return SSM_OK;          // a frame without a block: the cleared counts are the result, no output is touched
    const unsigned char *pa = static_cast<const unsigned char *>(a), *pb = static_cast<const unsigned char *>(b);
    with_sample(sample_bytes, [&](auto s) {
        with_layout(layout, [&](auto lay) {
            SSM_LAUNCH((static_paste_kernel<decltype(s), decltype(lay)::value>), dim3((unsigned)groups, N), dim3(LANES), 0, (hipStream_t)stream, pa, pb,
                       stride_a, stride_b, static_cast<unsigned char *>(out), stride_out, T, W, pl.cw, pl.luma(), pl.chroma(), (unsigned)nbx,
                       (unsigned)blocks, lo, counts);
        });
    });
    return ssm::check_launch("ssm_static_paste_fwd");
}

// ssm_flow_paste_fwd and ssm_flow_mix_fwd refuse in the order of their header sections - pointers, N and T, the entry's own scalars (split;
// den, then the k_j), and from there on as one (flow_block_call): the frame, K, the strides of a and b, of out, of the masks, 2-byte
// alignment, overlap, counts, the grid - and only then queue the clear and, for a frame that has blocks, the one launch.
struct FlowBlockGrid {
    YuvPlanes pl;
    long long nbx, blocks, groups;          // blocks per row, blocks, strips of PASTE_BLOCKS x PASTE_STEPS of them
};

static int flow_block_given(const char *name, const void *a, const void *b, const void *out, const void *mask, const void *counts, int N, int T) {
    SSM_REQUIRE(a && b && out && mask && counts, "%s: null pointer", name);
    SSM_REQUIRE(N > 0 && N <= 65535, "%s: N=%d outside 1..65535", name, N);
    SSM_REQUIRE(T > 0 && T <= 65535, "%s: T=%d outside 1..65535", name, T);
    return SSM_OK;
}

static int flow_block_call(const char *name, const void *a, const void *b, long long stride_a, long long stride_b, const void *out,
                           long long stride_out, int N, int T, int H, int W, int layout, int sample_bytes, const unsigned char *mask,
                           long long stride_mask, int K, const unsigned long long *counts, FlowBlockGrid *g) {
    if (const int e = check_frame(name, H, W, layout, sample_bytes)) return e;
    SSM_REQUIRE(K >= 0 && K <= 64, "%s: K=%d outside 0..64", name, K);
    const YuvPlanes pl = yuv_planes(H, W, layout);
    const long long fb = pl.frame() * sample_bytes, outs = (long long)N * T, mb = 2 * pl.luma();
    const PairEntry k = {name, "frame", fb};
    SSM_REQUIRE(N == 1 || (std::llabs(stride_a) >= fb && std::llabs(stride_b) >= fb), "%s: strides %lld (a), %lld (b) shorter than the frame's %lld bytes",
                name, stride_a, stride_b, fb);
    SSM_REQUIRE(outs == 1 || std::llabs(stride_out) >= fb, "%s: stride %lld (out) shorter than the frame's %lld bytes", name, stride_out, fb);
    SSM_REQUIRE(N == 1 || std::llabs(stride_mask) >= mb, "%s: stride %lld (mask) shorter than a pair's two planes, %lld bytes", name, stride_mask, mb);
    if (sample_bytes == 2) {
        const auto odd = [](const void *p) { return reinterpret_cast<size_t>(p) % 2 != 0; };
        SSM_REQUIRE(!odd(a) && !odd(b) && !odd(out), "%s: a payload of 2-byte samples (a, b or out) is not 2-byte aligned", name);
        SSM_REQUIRE(stride_a % 2 == 0 && stride_b % 2 == 0 && stride_out % 2 == 0, "%s: strides %lld (a), %lld (b), %lld (out) of 2-byte samples must be even",
                    name, stride_a, stride_b, stride_out);
    }
    long long o0, o1, a0, a1, b0, b1, m0, m1;
    rows_range(out, stride_out, outs, fb, &o0, &o1);
    rows_range(a, stride_a, N, fb, &a0, &a1);
    rows_range(b, stride_b, N, fb, &b0, &b1);
    rows_range(mask, stride_mask, N, mb, &m0, &m1);
    SSM_REQUIRE((a1 <= o0 || o1 <= a0) && (b1 <= o0 || o1 <= b0) && (m1 <= o0 || o1 <= m0), "%s: out overlaps a, b or mask", name);
    SSM_REQUIRE(reinterpret_cast<size_t>(counts) % 8 == 0, "%s: counts is not 8-byte aligned", name);
    const long long nbx = W >> 3, blocks = nbx * (H >> 3), strip = PASTE_BLOCKS * PASTE_STEPS;
    *g = {pl, nbx, blocks, (blocks + strip - 1) / strip};
    return grid_fits(k, g->groups);
}

extern "C" int ssm_flow_paste_fwd(const void *a, const void *b, long long stride_a, long long stride_b, void *out, long long stride_out, int N,
                                  int T, int split, int H, int W, int layout, int sample_bytes, const unsigned char *mask, long long stride_mask,
                                  int K, unsigned long long *counts, void *stream) {
    const char *name = "flow_paste";
    if (const int e = flow_block_given(name, a, b, out, mask, counts, N, T)) return e;
    SSM_REQUIRE(split >= 0 && split <= T, "%s: split=%d outside 0..T=%d", name, split, T);
    FlowBlockGrid g;
    if (const int e = flow_block_call(name, a, b, stride_a, stride_b, out, stride_out, N, T, H, W, layout, sample_bytes, mask, stride_mask, K,
                                      counts, &g))
        return e;
    if (const int e = clear_sums(name, counts, (size_t)N, stream)) return e;
    if (g.blocks == 0) return SSM_OK;          // a frame without a block: the cleared counts are the result, no output is touched
    const unsigned char *pa = static_cast<const unsigned char *>(a), *pb = static_cast<const unsigned char *>(b);
    with_sample(sample_bytes, [&](auto s) {
        with_layout(layout, [&](auto lay) {
            SSM_LAUNCH((flow_paste_kernel<decltype(s), decltype(lay)::value>), dim3((unsigned)g.groups, N), dim3(LANES), 0, (hipStream_t)stream, pa,
                       pb, stride_a, stride_b, static_cast<unsigned char *>(out), stride_out, T, split, W, g.pl.cw, g.pl.luma(), g.pl.chroma(),
                       (unsigned)g.nbx, (unsigned)g.blocks, mask, stride_mask, (unsigned)K, counts);
        });
    });
    return ssm::check_launch("ssm_flow_paste_fwd");
}

extern "C" int ssm_flow_mix_fwd(const void *a, const void *b, long long stride_a, long long stride_b, void *out, long long stride_out, int N,
                                int T, int num0, int num_step, int den, int H, int W, int layout, int sample_bytes, const unsigned char *mask,
                                long long stride_mask, int K, unsigned long long *counts, void *stream) {
    const char *name = "flow_mix";
    if (const int e = flow_block_given(name, a, b, out, mask, counts, N, T)) return e;
    SSM_REQUIRE(den >= 2 && den <= 65535, "%s: den=%d outside 2..65535", name, den);
    const long long k_last = (long long)num0 + (long long)(T - 1) * num_step;
    SSM_REQUIRE(num0 >= 0 && num0 <= den && k_last >= 0 && k_last <= den, "%s: k = %d + j * %d leaves 0..den=%d within T=%d outputs", name, num0,
                num_step, den, T);
    FlowBlockGrid g;
    if (const int e = flow_block_call(name, a, b, stride_a, stride_b, out, stride_out, N, T, H, W, layout, sample_bytes, mask, stride_mask, K,
                                      counts, &g))
        return e;
    if (const int e = clear_sums(name, counts, (size_t)N, stream)) return e;
    if (g.blocks == 0) return SSM_OK;          // a frame without a block: the cleared counts are the result, no output is touched
    const MixDivisor d = mix_divisor(den);
    const unsigned char *pa = static_cast<const unsigned char *>(a), *pb = static_cast<const unsigned char *>(b);
    with_sample(sample_bytes, [&](auto s) {
        with_layout(layout, [&](auto lay) {
            SSM_LAUNCH((flow_mix_kernel<decltype(s), decltype(lay)::value>), dim3((unsigned)g.groups, N), dim3(LANES), 0, (hipStream_t)stream, pa, pb,
                       stride_a, stride_b, static_cast<unsigned char *>(out), stride_out, T, num0, num_step, den, d, W, g.pl.cw, g.pl.luma(),
                       g.pl.chroma(), (unsigned)g.nbx, (unsigned)g.blocks, mask, stride_mask, (unsigned)K, counts);
        });
    });
    return ssm::check_launch("ssm_flow_mix_fwd");
}

// ---- interlaced clips -------------------------------------------------------------------------------------------------------------------
// ssm_fields_split_fwd and ssm_fields_weave_fwd refuse in one order: pointers, N, the frame (size, layout, sample width), the rows the
// layout asks of an interlaced frame, the grid, parity0 and fill, 2-byte alignment, strides, overlap - and only then queue the one launch.
static int fields_frame(const char *name, int N, int H, int W, int layout, int sample_bytes, FieldGeom *g) {
    SSM_REQUIRE(N > 0 && N <= 65535, "%s: N=%d outside 1..65535", name, N);
    if (const int e = check_frame(name, H, W, layout, sample_bytes)) return e;
    const bool c420 = layout == SSM_YUV_420_CENTRED || layout == SSM_YUV_420_COSITED;
    SSM_REQUIRE(H % 2 == 0, "%s: an interlaced frame has an even number of rows (H=%d)", name, H);
    SSM_REQUIRE(!c420 || H % 4 == 0, "%s: an interlaced 4:2:0 frame has a multiple of 4 rows, two chroma fields of H/4 (H=%d)", name, H);
    const YuvPlanes pl = yuv_planes(H, W, layout);
    const long long per = 16 / sample_bytes;
    long long at = 0, pieces = 0;
    for (int p = 0; p < 3; ++p) {
        const long long rows = p ? pl.ch : pl.h, cols = p ? pl.cw : pl.w, pp = (cols + per - 1) / per;
        g->rows[p] = (unsigned)rows, g->cols[p] = (unsigned)cols, g->pieces[p] = (unsigned)pp;
        g->off[p] = at;
        at += rows * cols;
        SSM_REQUIRE(pieces + rows * pp <= 2147483647ll, "%s: a frame of %lld bytes is more than the grid takes", name, pl.frame() * sample_bytes);
        g->start[p] = (unsigned)pieces;
        pieces += rows * pp;
    }
    g->total = (unsigned)pieces;
    return SSM_OK;
}

static bool apart(long long a0, long long a1, long long b0, long long b1) { return a1 <= b0 || b1 <= a0; }

extern "C" int ssm_fields_split_fwd(const void *frames, void *fields, int N, int H, int W, int layout, int sample_bytes, void *stream) {
    const char *name = "fields_split";
    SSM_REQUIRE(frames && fields, "%s: null pointer", name);
    FieldGeom g;
    if (const int e = fields_frame(name, N, H, W, layout, sample_bytes, &g)) return e;
    const auto odd = [](const void *p) { return reinterpret_cast<size_t>(p) % 2 != 0; };
    SSM_REQUIRE(sample_bytes == 1 || (!odd(frames) && !odd(fields)), "%s: a payload of 2-byte samples (frames or fields) is not 2-byte aligned", name);
    const long long fb = yuv_planes(H, W, layout).frame() * sample_bytes;
    long long i0, i1, o0, o1;
    rows_range(frames, fb, N, fb, &i0, &i1);
    rows_range(fields, fb, N, fb, &o0, &o1);
    SSM_REQUIRE(apart(i0, i1, o0, o1), "%s: fields overlaps frames", name);
    const unsigned groups = (g.total + LANES * CHUNKS - 1) / (LANES * CHUNKS);
    with_sample(sample_bytes, [&](auto s) {
        SSM_LAUNCH(fields_split_kernel<decltype(s)>, dim3(groups, N), dim3(LANES), 0, (hipStream_t)stream, static_cast<const unsigned char *>(frames),
                   static_cast<unsigned char *>(fields), fb, g);
    });
    return ssm::check_launch("ssm_fields_split_fwd");
}

extern "C" int ssm_fields_weave_fwd(const void *kept, long long stride_kept, const void *made, long long stride_made, void *frames,
                                    long long stride_frames, int N, int H, int W, int layout, int sample_bytes, int parity0, int fill, void *stream) {
    const char *name = "fields_weave";
    SSM_REQUIRE(kept && frames && (made || fill == 1), "%s: null pointer", name);
    FieldGeom g;
    if (const int e = fields_frame(name, N, H, W, layout, sample_bytes, &g)) return e;
    SSM_REQUIRE(parity0 == 0 || parity0 == 1, "%s: parity0 %d not in {0, 1}", name, parity0);
    SSM_REQUIRE(fill == 0 || fill == 1, "%s: fill %d not in {0, 1}", name, fill);
    if (fill) made = nullptr, stride_made = 0;          // not read: what it points at, and how, is not looked at
    const long long fb = yuv_planes(H, W, layout).frame() * sample_bytes, hb = fb / 2;
    if (sample_bytes == 2) {
        const auto odd = [](const void *p) { return reinterpret_cast<size_t>(p) % 2 != 0; };
        SSM_REQUIRE(!odd(kept) && !odd(made) && !odd(frames), "%s: a payload of 2-byte samples (kept, made or frames) is not 2-byte aligned", name);
        SSM_REQUIRE(N == 1 || (stride_kept % 2 == 0 && stride_made % 2 == 0 && stride_frames % 2 == 0),
                    "%s: strides %lld (kept), %lld (made), %lld (frames) of 2-byte samples must be even", name, stride_kept, stride_made, stride_frames);
    }
    if (N == 1) stride_kept = stride_made = stride_frames = 0;          // the stride of a single payload names nothing
    SSM_REQUIRE(N == 1 || (std::llabs(stride_kept) >= hb && (fill || std::llabs(stride_made) >= hb)),
                "%s: strides %lld (kept), %lld (made) shorter than the field's %lld bytes", name, stride_kept, stride_made, hb);
    SSM_REQUIRE(N == 1 || std::llabs(stride_frames) >= fb, "%s: stride %lld (frames) shorter than the frame's %lld bytes", name, stride_frames, fb);
    long long k0, k1, m0 = 0, m1 = 0, o0, o1;
    rows_range(kept, stride_kept, N, hb, &k0, &k1);
    if (made) rows_range(made, stride_made, N, hb, &m0, &m1);
    rows_range(frames, stride_frames, N, fb, &o0, &o1);
    SSM_REQUIRE(apart(k0, k1, o0, o1) && (!made || apart(m0, m1, o0, o1)), "%s: frames overlaps kept or made", name);
    const unsigned groups = (g.total + LANES * CHUNKS - 1) / (LANES * CHUNKS);
    with_sample(sample_bytes, [&](auto s) {
        SSM_LAUNCH(fields_weave_kernel<decltype(s)>, dim3(groups, N), dim3(LANES), 0, (hipStream_t)stream, static_cast<const unsigned char *>(kept),
                   stride_kept, static_cast<const unsigned char *>(made), stride_made, static_cast<unsigned char *>(frames), stride_frames, g,
                   parity0, fill);
    });
    return ssm::check_launch("ssm_fields_weave_fwd");
}

// ---- letterboxed clips -------------------------------------------------------------------------------------------------------------------
// ssm_luma_counts_fwd refuses in the order of ssm_block_sad_fwd - pointers, N, the plane, sample_bytes, the stride, 2-byte alignment, limit,
// the arrays' alignment, the grid - and only then queues its two clears and the launch.
extern "C" int ssm_luma_counts_fwd(const void *frames, long long stride, int N, int H, int W, int sample_bytes, int limit, unsigned *rows,
                                   unsigned *cols, void *stream) {
    const char *name = "luma_counts";
    SSM_REQUIRE(frames && rows && cols, "%s: null pointer", name);
    SSM_REQUIRE(N > 0 && N <= 65535, "%s: N=%d outside 1..65535", name, N);
    SSM_REQUIRE(H > 0 && W > 0, "%s: bad plane size %dx%d", name, H, W);
    SSM_REQUIRE(sample_bytes == 1 || sample_bytes == 2, "%s: sample_bytes %d not in {1, 2}", name, sample_bytes);
    const long long plane = (long long)H * W * sample_bytes;
    SSM_REQUIRE(N == 1 || std::llabs(stride) >= plane, "%s: stride %lld shorter than the plane's %lld bytes", name, stride, plane);
    if (sample_bytes == 2) {
        SSM_REQUIRE(reinterpret_cast<size_t>(frames) % 2 == 0, "%s: a plane of 2-byte samples is not 2-byte aligned", name);
        SSM_REQUIRE(N == 1 || stride % 2 == 0, "%s: stride %lld of 2-byte samples must be even", name, stride);
    }
    SSM_REQUIRE(limit >= 0 && limit <= 65535, "%s: limit=%d outside 0..65535", name, limit);
    SSM_REQUIRE(reinterpret_cast<size_t>(rows) % 4 == 0 && reinterpret_cast<size_t>(cols) % 4 == 0, "%s: rows or cols is not 4-byte aligned", name);
    const long long gx = ((long long)W + COUNT_COLS - 1) / COUNT_COLS, gy = ((long long)H + COUNT_BAND - 1) / COUNT_BAND;
    SSM_REQUIRE(gy <= 65535, "%s: a plane of %d rows is more than the grid takes", name, H);
    if (N == 1) stride = 0;          // the stride of a single plane names nothing
    const hipError_t e0 = ssm::memset_async(rows, 0, sizeof(unsigned) * (size_t)N * (size_t)H, (hipStream_t)stream);
    const hipError_t e1 = e0 != hipSuccess ? e0 : ssm::memset_async(cols, 0, sizeof(unsigned) * (size_t)N * (size_t)W, (hipStream_t)stream);
    if (e1 != hipSuccess) {
        ssm::set_error("%s: memset failed: %s", name, hipGetErrorString(e1));
        return SSM_E_LAUNCH;
    }
    with_sample(sample_bytes, [&](auto s) {
        SSM_LAUNCH(luma_counts_kernel<decltype(s)>, dim3((unsigned)gx, (unsigned)gy, N), dim3(LANES), 0, (hipStream_t)stream,
                   static_cast<const unsigned char *>(frames), stride, H, W, (unsigned)limit, rows, cols);
    });
    return ssm::check_launch("ssm_luma_counts_fwd");
}

// ssm_window_cut_fwd refuses in one order: pointers, N, the frame (size, layout, sample width), the rectangle (inside the frame, then
// aligned for the layout), the grid, 2-byte alignment, strides, overlap - and only then queues the one launch.
extern "C" int ssm_window_cut_fwd(const void *frames, long long stride_in, void *windows, long long stride_out, int N, int H, int W, int y0, int x0,
                                  int h, int w, int layout, int sample_bytes, void *stream) {
    const char *name = "window_cut";
    SSM_REQUIRE(frames && windows, "%s: null pointer", name);
    SSM_REQUIRE(N > 0 && N <= 65535, "%s: N=%d outside 1..65535", name, N);
    if (const int e = check_frame(name, H, W, layout, sample_bytes)) return e;
    SSM_REQUIRE(h > 0 && w > 0 && y0 >= 0 && x0 >= 0 && (long long)y0 + h <= H && (long long)x0 + w <= W,
                "%s: the window %dx%d at (%d,%d) (h x w at y, x) lies outside the %dx%d frame", name, h, w, y0, x0, H, W);
    const int ay = (layout == SSM_YUV_420_CENTRED || layout == SSM_YUV_420_COSITED) ? 2 : 1, ax = layout == SSM_YUV_444 ? 1 : 2;
    SSM_REQUIRE(y0 % ay == 0 && x0 % ax == 0 && ((y0 + h) % ay == 0 || y0 + h == H) && ((x0 + w) % ax == 0 || x0 + w == W),
                "%s: the window %dx%d at (%d,%d) is not aligned to (%d,%d) rows and columns, as layout %d asks: its origin a multiple, its far "
                "edges a multiple or the frame's own", name, h, w, y0, x0, ay, ax, layout);
    const YuvPlanes fr = yuv_planes(H, W, layout), wi = yuv_planes(h, w, layout);
    WindowGeom g;
    const long long per = 16 / sample_bytes;
    long long pieces = 0;
    for (int p = 0; p < 3; ++p) {
        const long long rows = p ? wi.ch : wi.h, cols = p ? wi.cw : wi.w, pp = (cols + per - 1) / per;
        g.rows[p] = (unsigned)rows, g.cols[p] = (unsigned)cols, g.pieces[p] = (unsigned)pp;
        g.dst[p] = p == 0 ? 0 : wi.luma() + (p - 1) * wi.chroma();
        g.pitch[p] = p ? fr.cw : fr.w;
        g.src[p] = (p == 0 ? 0 : fr.luma() + (p - 1) * fr.chroma()) + (long long)(p ? y0 / ay : y0) * g.pitch[p] + (p ? x0 / ax : x0);
        SSM_REQUIRE(pieces + rows * pp <= 2147483647ll, "%s: a window of %lld bytes is more than the grid takes", name, wi.frame() * sample_bytes);
        g.start[p] = (unsigned)pieces;
        pieces += rows * pp;
    }
    g.total = (unsigned)pieces;
    const long long fb = fr.frame() * sample_bytes, wb = wi.frame() * sample_bytes;
    if (sample_bytes == 2) {
        const auto odd = [](const void *p) { return reinterpret_cast<size_t>(p) % 2 != 0; };
        SSM_REQUIRE(!odd(frames) && !odd(windows), "%s: a payload of 2-byte samples (frames or windows) is not 2-byte aligned", name);
        SSM_REQUIRE(N == 1 || (stride_in % 2 == 0 && stride_out % 2 == 0), "%s: strides %lld (frames), %lld (windows) of 2-byte samples must be even",
                    name, stride_in, stride_out);
    }
    if (N == 1) stride_in = stride_out = 0;          // the stride of a single payload names nothing
    SSM_REQUIRE(N == 1 || std::llabs(stride_in) >= fb, "%s: stride %lld (frames) shorter than the frame's %lld bytes", name, stride_in, fb);
    SSM_REQUIRE(N == 1 || std::llabs(stride_out) >= wb, "%s: stride %lld (windows) shorter than the window's %lld bytes", name, stride_out, wb);
    long long i0, i1, o0, o1;
    rows_range(frames, stride_in, N, fb, &i0, &i1);
    rows_range(windows, stride_out, N, wb, &o0, &o1);
    SSM_REQUIRE(apart(i0, i1, o0, o1), "%s: windows overlaps frames", name);
    const unsigned groups = (g.total + LANES * CHUNKS - 1) / (LANES * CHUNKS);
    with_sample(sample_bytes, [&](auto s) {
        SSM_LAUNCH(window_cut_kernel<decltype(s)>, dim3(groups, N), dim3(LANES), 0, (hipStream_t)stream, static_cast<const unsigned char *>(frames),
                   stride_in, static_cast<unsigned char *>(windows), stride_out, g);
    });
    return ssm::check_launch("ssm_window_cut_fwd");
}
