// Optical-flow evaluation on the device: the end-point-error record of scripts/evaluate_optical_flow_results.py:18-28 (compute_metrics)
// / scripts/utils/flo_utils.py:86-138 (flow_error), and the Middlebury colour coding of scripts/utils/flo_utils.py:141-272
// (flow_to_image + compute_color + make_color_wheel).  Both read a planar fp32 flow [N,2,*,*] behind an ssm_view (channel 0 = u,
// 1 = v), cropped at (top, left) to H x W, where stage 1 left it.  Two deterministic launches each, in the manner of ssm_metrics.hip:
//   flow_epe_kernel     FL_PIX consecutive pixels of one field per workgroup: the per-pixel error in numpy's float32 arithmetic, a
//                       fixed-order workgroup sum of (error in fp64, error > 3, counted) into the chunk's slot of the caller's workspace;
//   flow_epe_finish     one workgroup per field: the field's slots summed in a fixed order into out[n][3];
//   flow_maxrad_kernel  the chunk's maximum fp32 radius into its slot (a float max does not depend on the order: exact);
//   flow_rgb_kernel     every workgroup takes the maximum over its field's slots, then normalises, looks the angle up in the colour
//                       wheel, interpolates and writes uint8 RGB - in fp64, as the reference's map runs on numpy >= 2.
// And the forward-backward consistency of the two fields stage 1 leaves side by side (F01 | F10, four planes), which has no reference
// code: its definition stands in include/ssm_hip.h and its yardstick is ssm_amd.flow_eval.flow_consistency_host.
//   flow_consistency_kernel  FL_PIX consecutive pixels of one pair per workgroup, both directions: per pixel the state (consistent,
//                            inconsistent, leaves) in fp32, a fixed-order workgroup sum of the three counts (integers) and the residuals
//                            (fp64) per direction into the chunk's slot; optionally the state into a uint8 mask;
//   flow_consistency_finish  one workgroup per pair: the pair's slots summed in a fixed order into out[n][2][4].
// Every partial result has one writer and is combined in a fixed order, so the bits depend only on the field's values and size, not
// on N, the stream or the run.
// NO CONTRACTION.  hipcc fuses a*b + c into one fma by default; numpy rounds every operation.  The two decisions of this file - error
// > 3 and radius <= 1 (the colour map's one discontinuity, and the pixel of maximum radius sits right on it) - must be the reference's
// decisions bit for bit.  HIP's __fmul_rn / __fadd_rn / __dmul_rn / __dadd_rn do not help: without OCML_BASIC_ROUNDED_OPERATIONS they
// are the plain operators (and fuse like them), and __fsqrt_rn is the hardware's 1-ulp root, which moved the EPE sum by 1e-8.  So
// contraction is off for the whole file - by the pragma below and by the Makefile's -ffp-contract=off - and the fp32 root is
// __builtin_sqrtf, which hipcc rounds correctly by default (-fhip-fp32-correctly-rounded-divide-sqrt); the fp64 root is correctly rounded.
#include "ssm_common.h"
#include "ssm_device.h"

#pragma clang fp contract(off)

namespace {

constexpr int FL_THREADS = 256;
constexpr int FL_PER = 8;                          // pixels per thread
constexpr int FL_PIX = FL_THREADS * FL_PER;        // pixels per workgroup (one workspace slot)
constexpr float FL_UNKNOWN = 1e7f;                 // UNKNOWN_FLOW_THRESH (flo_utils.py:9)

inline int chunks_of(int H, int W) { return (int)(((long long)H * W + FL_PIX - 1) / FL_PIX); }

// ---- make_color_wheel (flo_utils.py:225-272), every entry already divided by 255 in double (compute_color: tmp[k] / 255) -----------
constexpr int FL_NCOLS = 55;          // RY + YG + GC + CB + BM + MR
struct Wheel {
    double c[FL_NCOLS][3];
};
// floor(255 * i / n) of the reference's float64 expression: 255 * i is exact and a quotient that is not an integer lies at least 1/15
// from one, so the integer division below is that floor
constexpr double ramp(int i, int n) { return (double)((255 * i) / n); }
constexpr Wheel make_wheel() {
    constexpr int RY = 15, YG = 6, GC = 4, CB = 11, BM = 13, MR = 6;
    static_assert(RY + YG + GC + CB + BM + MR == FL_NCOLS, "wheel size");
    Wheel w{};
    int col = 0;
    for (int i = 0; i < RY; ++i) w.c[col + i][0] = 255.0, w.c[col + i][1] = ramp(i, RY);
    col += RY;
    for (int i = 0; i < YG; ++i) w.c[col + i][0] = 255.0 - ramp(i, YG), w.c[col + i][1] = 255.0;
    col += YG;
    for (int i = 0; i < GC; ++i) w.c[col + i][1] = 255.0, w.c[col + i][2] = ramp(i, GC);
    col += GC;
    for (int i = 0; i < CB; ++i) w.c[col + i][1] = 255.0 - ramp(i, CB), w.c[col + i][2] = 255.0;
    col += CB;
    for (int i = 0; i < BM; ++i) w.c[col + i][2] = 255.0, w.c[col + i][0] = ramp(i, BM);
    col += BM;
    for (int i = 0; i < MR; ++i) w.c[col + i][2] = 255.0 - ramp(i, MR), w.c[col + i][0] = 255.0;
    for (int k = 0; k < FL_NCOLS; ++k)
        for (int c = 0; c < 3; ++c) w.c[k][c] = w.c[k][c] / 255.0;
    return w;
}
__constant__ Wheel c_wheel = make_wheel();

// pixel p of the H x W crop of field n: its offset inside the view
__device__ __forceinline__ size_t flow_off(const ssm_view &f, int n, int p, int W, int top, int left) {
    const int y = p / W, x = p - y * W;
    return (size_t)n * f.sb + (size_t)(top + y) * f.sh + (size_t)(left + x);
}

// ---- end-point error ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FL_THREADS) void flow_epe_kernel(ssm_view flow, const float *__restrict__ gt, int HW, int W, int top, int left,
                                                              int mode, double *__restrict__ ws) {
    __shared__ double red_e[FL_THREADS];
    __shared__ unsigned red_c[2][FL_THREADS];
    const int tid = threadIdx.x, n = blockIdx.y;
    double e = 0.0;
    unsigned over = 0, cnt = 0;
#pragma unroll
    for (int i = 0; i < FL_PER; ++i) {
        const long long pl = (long long)blockIdx.x * FL_PIX + i * FL_THREADS + tid;
        if (pl >= HW) continue;
        const int p = (int)pl;
        const size_t off = flow_off(flow, n, p, W, top, left);
        const float u = flow.ptr[off], v = flow.ptr[off + flow.sc];
        const f32x2 g = *reinterpret_cast<const f32x2 *>(gt + ((size_t)n * HW + p) * 2);
        // mode 1: flow_error's mask - ground truth unknown in either component, or zero in both, does not count
        const bool unknown = fabsf(g.x) > FL_UNKNOWN || fabsf(g.y) > FL_UNKNOWN;
        const bool counted = mode == 0 || (!unknown && (fabsf(g.x) > 0.0f || fabsf(g.y) > 0.0f));
        // sqrt(sum((gt - flow) ** 2)) on float32 arrays: each product, the sum and the root rounded once
        const float dx = g.x - u, dy = g.y - v;
        const float err = __builtin_sqrtf(dx * dx + dy * dy);
        if (counted) {
            e += (double)err;
            over += err > 3.0f ? 1u : 0u;
            cnt += 1u;
        }
    }
    red_e[tid] = e;
    red_c[0][tid] = over;
    red_c[1][tid] = cnt;
    __syncthreads();
    for (int s = FL_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) {
            red_e[tid] += red_e[tid + s];
            red_c[0][tid] += red_c[0][tid + s];
            red_c[1][tid] += red_c[1][tid + s];
        }
        __syncthreads();
    }
    if (tid == 0) {
        double *slot = ws + ((size_t)n * gridDim.x + blockIdx.x) * 3;
        slot[0] = red_e[0];
        slot[1] = (double)red_c[0][0];
        slot[2] = (double)red_c[1][0];
    }
}

__global__ __launch_bounds__(FL_THREADS) void flow_epe_finish(const double *__restrict__ ws, int chunks, double *__restrict__ out) {
    __shared__ double red[3][FL_THREADS];
    const int tid = threadIdx.x, n = blockIdx.x;
    double a[3] = {0.0, 0.0, 0.0};
    for (int t = tid; t < chunks; t += FL_THREADS) {
#pragma unroll
        for (int m = 0; m < 3; ++m) a[m] += ws[((size_t)n * chunks + t) * 3 + m];
    }
#pragma unroll
    for (int m = 0; m < 3; ++m) red[m][tid] = a[m];
    __syncthreads();
    for (int s = FL_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) {
#pragma unroll
            for (int m = 0; m < 3; ++m) red[m][tid] += red[m][tid + s];
        }
        __syncthreads();
    }
    if (tid < 3) out[(size_t)n * 3 + tid] = red[tid][0];
}

// ---- colour coding -----------------------------------------------------------------------------------------------------------------
// flow_to_image's first step (flo_utils.py:155-157): a pixel unknown in either component is flow 0 (and black in the end)
__device__ __forceinline__ bool load_uv(const ssm_view &f, size_t off, float &u, float &v) {
    u = f.ptr[off];
    v = f.ptr[off + f.sc];
    const bool unknown = fabsf(u) > FL_UNKNOWN || fabsf(v) > FL_UNKNOWN;
    if (unknown) u = v = 0.0f;
    return unknown;
}

// Plain max of two radii.  A NaN never wins `a > b`, so flow_maxrad_kernel replaces a NaN radius by +inf BEFORE it calls this, and +inf
// then stands for "the field holds a NaN": a radius is never +inf by itself (|u|, |v| <= 1e7 after the unknown test)
__device__ __forceinline__ float rad_max(float a, float b) { return a > b ? a : b; }

__global__ __launch_bounds__(FL_THREADS) void flow_maxrad_kernel(ssm_view flow, int HW, int W, int top, int left, float *__restrict__ ws) {
    __shared__ float red[FL_THREADS];
    const int tid = threadIdx.x, n = blockIdx.y;
    float m = -1.0f;                                  // max(-1, np.max(rad)), flo_utils.py:166
#pragma unroll
    for (int i = 0; i < FL_PER; ++i) {
        const long long pl = (long long)blockIdx.x * FL_PIX + i * FL_THREADS + tid;
        if (pl >= HW) continue;
        float u, v;
        load_uv(flow, flow_off(flow, n, (int)pl, W, top, left), u, v);
        float r = __builtin_sqrtf(u * u + v * v);          // np.sqrt(u ** 2 + v ** 2) on float32
        if (r != r) r = __builtin_inff();
        m = rad_max(m, r);
    }
    red[tid] = m;
    __syncthreads();
    for (int s = FL_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] = rad_max(red[tid], red[tid + s]);
        __syncthreads();
    }
    if (tid == 0) ws[(size_t)n * gridDim.x + blockIdx.x] = red[0];
}

__global__ __launch_bounds__(FL_THREADS) void flow_rgb_kernel(ssm_view flow, int HW, int W, int top, int left, const float *__restrict__ ws,
                                                              unsigned char *__restrict__ rgb) {
    __shared__ float red[FL_THREADS];
    const int tid = threadIdx.x, n = blockIdx.y, chunks = gridDim.x;
    float m = -1.0f;
    for (int t = tid; t < chunks; t += FL_THREADS) m = rad_max(m, ws[(size_t)n * chunks + t]);
    red[tid] = m;
    __syncthreads();
    for (int s = FL_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] = rad_max(red[tid], red[tid + s]);
        __syncthreads();
    }
    // A NaN anywhere in the field makes np.max(rad) NaN, and Python's max(-1, nan) keeps its first argument: the reference then
    // divides by -1 + eps (flo_utils.py:166-171).  The +inf that stands for that NaN here selects the same -1.
    const float maxrad = red[0] == __builtin_inff() ? -1.0f : red[0];
    const double den = (double)maxrad + 2.220446049250313e-16;          // maxrad + np.finfo(float).eps, in float64
    const double pi = 3.141592653589793;
#pragma unroll 1
    for (int i = 0; i < FL_PER; ++i) {
        const long long pl = (long long)blockIdx.x * FL_PIX + i * FL_THREADS + tid;
        if (pl >= HW) continue;
        const int p = (int)pl;
        float uf, vf;
        const bool unknown = load_uv(flow, flow_off(flow, n, p, W, top, left), uf, vf);
        double un = (double)uf / den, vn = (double)vf / den;
        const bool isnan = un != un || vn != vn;          // compute_color: nanIdx -> flow 0, colour * 0
        if (isnan) un = vn = 0.0;
        const double rad = __builtin_sqrt(un * un + vn * vn);
        const double a = atan2(-vn, -un) / pi;
        const double fk = (a + 1.0) / 2.0 * (double)(FL_NCOLS - 1) + 1.0;
        int k0 = (int)floor(fk);
        k0 = k0 < 1 ? 1 : (k0 > FL_NCOLS ? FL_NCOLS : k0);          // fk is in [1, 55]; the clamp only keeps the table reads inside
        const int k1 = k0 == FL_NCOLS ? 1 : k0 + 1;
        const double f = fk - (double)k0;
        unsigned char *dst = rgb + ((size_t)n * HW + p) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double col0 = c_wheel.c[k0 - 1][c], col1 = c_wheel.c[k1 - 1][c];
            double col = (1.0 - f) * col0 + f * col1;
            if (rad <= 1.0)
                col = 1.0 - rad * (1.0 - col);
            else
                col = col * 0.75;
            const double level = floor(255.0 * col);
            dst[c] = (unknown || isnan) ? (unsigned char)0 : (unsigned char)(int)level;
        }
    }
}

// ---- forward-backward consistency ------------------------------------------------------------------------------------------------------
// The definition of include/ssm_hip.h (ssm_flow_consistency_fwd), one rounded fp32 operation per step: pixel (x, y) of the crop follows
// F to (px, py); where that point stays on the crop, G is sampled there bilinearly - taps inside the crop only, the canvas around it
// holds whatever the U-Net left - and F + G' should vanish.  Returns 0 consistent, 1 inconsistent, 2 leaves; `residual` only for 0 / 1.
// fu, fv, gu, gv: the planes of the two fields at the crop's origin.
constexpr int FC_WORDS = 8;                        // a workspace slot: [direction][judged, inconsistent, leaves] as integers, then [direction] fp64 residual sums

__device__ __forceinline__ unsigned fc_pixel(float u, float v, const float *__restrict__ gu, const float *__restrict__ gv, int sh, int x,
                                             int y, int H, int W, float alpha, float beta, float &residual) {
    const float px = (float)x + u, py = (float)y + v;
    if (!(px >= 0.0f && px <= (float)(W - 1) && py >= 0.0f && py <= (float)(H - 1))) return 2u;          // a NaN leaves
    const float x0 = floorf(px), y0 = floorf(py);
    const float fx = px - x0, fy = py - y0;
    const int xi0 = (int)x0, yi0 = (int)y0;          // in [0, W - 1] x [0, H - 1] by the test above
    const int xi1 = xi0 + 1 < W ? xi0 + 1 : W - 1, yi1 = yi0 + 1 < H ? yi0 + 1 : H - 1;
    const size_t r0 = (size_t)yi0 * sh, r1 = (size_t)yi1 * sh;
    float s[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const float *g = c == 0 ? gu : gv;
        const float g00 = g[r0 + xi0], g01 = g[r0 + xi1], g10 = g[r1 + xi0], g11 = g[r1 + xi1];
        const float a = g00 + fx * (g01 - g00);
        const float b = g10 + fx * (g11 - g10);
        s[c] = a + fy * (b - a);
    }
    const float rx = u + s[0], ry = v + s[1];
    const float e2 = rx * rx + ry * ry;
    const float m2 = ((u * u + v * v) + s[0] * s[0]) + s[1] * s[1];
    residual = __builtin_sqrtf(e2);
    return e2 > alpha * m2 + beta ? 1u : 0u;
}

// FL_PIX consecutive pixels of one pair per workgroup, lane = pixel along x: the four plane reads of a wave are contiguous row segments,
// the gathers of the other field land a few pixels from them.  Both directions of a pixel in one thread; a fixed-order workgroup sum
// into the chunk's slot.
__global__ __launch_bounds__(FL_THREADS) void flow_consistency_kernel(ssm_view flow4, int HW, int H, int W, int top, int left, float alpha,
                                                                      float beta, unsigned long long *__restrict__ ws,
                                                                      unsigned char *__restrict__ mask) {
    __shared__ double red_e[2][FL_THREADS];
    __shared__ unsigned red_c[6][FL_THREADS];
    const int tid = threadIdx.x, n = blockIdx.y;
    const float *base = flow4.ptr + (size_t)n * flow4.sb + (size_t)top * flow4.sh + (size_t)left;
    const float *pl[4] = {base, base + flow4.sc, base + 2 * flow4.sc, base + 3 * flow4.sc};          // u01, v01, u10, v10
    double e[2] = {0.0, 0.0};
    unsigned cnt[2][3] = {{0, 0, 0}, {0, 0, 0}};
#pragma unroll 2
    for (int i = 0; i < FL_PER; ++i) {
        const long long p_ = (long long)blockIdx.x * FL_PIX + i * FL_THREADS + tid;
        if (p_ >= HW) continue;
        const int p = (int)p_, y = p / W, x = p - y * W;
        const size_t off = (size_t)y * flow4.sh + (size_t)x;
        const float f[4] = {pl[0][off], pl[1][off], pl[2][off], pl[3][off]};
#pragma unroll
        for (int d = 0; d < 2; ++d) {
            float res = 0.0f;
            const unsigned state = fc_pixel(f[2 * d], f[2 * d + 1], pl[2 - 2 * d], pl[3 - 2 * d], flow4.sh, x, y, H, W, alpha, beta, res);
            if (state != 2u) {
                e[d] += (double)res;
                cnt[d][0] += 1u;
                cnt[d][1] += state;
            } else {
                cnt[d][2] += 1u;
            }
            if (mask) mask[((size_t)n * 2 + d) * HW + p] = (unsigned char)state;
        }
    }
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        red_e[d][tid] = e[d];
#pragma unroll
        for (int m = 0; m < 3; ++m) red_c[3 * d + m][tid] = cnt[d][m];
    }
    __syncthreads();
    for (int s = FL_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) {
            red_e[0][tid] += red_e[0][tid + s];
            red_e[1][tid] += red_e[1][tid + s];
#pragma unroll
            for (int m = 0; m < 6; ++m) red_c[m][tid] += red_c[m][tid + s];
        }
        __syncthreads();
    }
    unsigned long long *slot = ws + ((size_t)n * gridDim.x + blockIdx.x) * FC_WORDS;
    if (tid < 6) slot[tid] = red_c[tid][0];
    if (tid == 6 || tid == 7) reinterpret_cast<double *>(slot)[tid] = red_e[tid - 6][0];
}

// one workgroup per pair: its slots summed in a fixed order - the counts as integers, the residuals in fp64 - into out[n][2][4]
__global__ __launch_bounds__(FL_THREADS) void flow_consistency_finish(const unsigned long long *__restrict__ ws, int chunks,
                                                                      double *__restrict__ out) {
    __shared__ unsigned long long red_c[6][FL_THREADS];
    __shared__ double red_e[2][FL_THREADS];
    const int tid = threadIdx.x, n = blockIdx.x;
    unsigned long long c[6] = {0, 0, 0, 0, 0, 0};
    double e[2] = {0.0, 0.0};
    for (int t = tid; t < chunks; t += FL_THREADS) {
        const unsigned long long *slot = ws + ((size_t)n * chunks + t) * FC_WORDS;
#pragma unroll
        for (int m = 0; m < 6; ++m) c[m] += slot[m];
        e[0] += reinterpret_cast<const double *>(slot)[6];
        e[1] += reinterpret_cast<const double *>(slot)[7];
    }
#pragma unroll
    for (int m = 0; m < 6; ++m) red_c[m][tid] = c[m];
    red_e[0][tid] = e[0];
    red_e[1][tid] = e[1];
    __syncthreads();
    for (int s = FL_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) {
#pragma unroll
            for (int m = 0; m < 6; ++m) red_c[m][tid] += red_c[m][tid + s];
            red_e[0][tid] += red_e[0][tid + s];
            red_e[1][tid] += red_e[1][tid + s];
        }
        __syncthreads();
    }
    if (tid < 2) {
        double *o = out + ((size_t)n * 2 + tid) * 4;
        o[0] = (double)red_c[3 * tid][0];
        o[1] = (double)red_c[3 * tid + 1][0];
        o[2] = (double)red_c[3 * tid + 2][0];
        o[3] = red_e[tid][0];
    }
}

int check_field(const char *who, ssm_view flow, int N, int H, int W, int top, int left) {
    SSM_REQUIRE(flow.ptr, "%s: null pointer (flow)", who);
    SSM_REQUIRE(N >= 1 && N <= 65535, "%s: N = %d outside [1, 65535]", who, N);
    SSM_REQUIRE(H >= 1 && W >= 1, "%s: %dx%d field", who, H, W);
    SSM_REQUIRE((long long)H * W <= (1LL << 30), "%s: %dx%d field too large", who, H, W);
    SSM_REQUIRE(top >= 0 && left >= 0, "%s: crop origin (%d, %d) is negative", who, top, left);
    SSM_REQUIRE(flow.sh >= left + W, "%s: row stride %d is shorter than left + W = %d", who, flow.sh, left + W);
    return SSM_OK;
}

}  // namespace

extern "C" size_t ssm_flow_metrics_workspace_bytes(int N, int H, int W) {
    if (N < 1 || H < 1 || W < 1) return 0;
    return (size_t)N * chunks_of(H, W) * 3 * sizeof(double);
}

extern "C" int ssm_flow_metrics_fwd(ssm_view flow, const float *gt_hw2, int N, int H, int W, int top, int left, int mode, void *workspace,
                                    size_t workspace_bytes, double *out, void *stream) {
    SSM_REQUIRE(gt_hw2 && workspace && out, "flow_metrics: null pointer");
    if (int rc = check_field("flow_metrics", flow, N, H, W, top, left)) return rc;
    SSM_REQUIRE(mode == 0 || mode == 1, "flow_metrics: mode %d (0 = every pixel, 1 = known, non-zero ground truth)", mode);
    SSM_REQUIRE((reinterpret_cast<size_t>(gt_hw2) & 7) == 0, "flow_metrics: gt_hw2 must be 8-byte aligned");
    const size_t need = ssm_flow_metrics_workspace_bytes(N, H, W);
    SSM_REQUIRE(workspace_bytes >= need, "flow_metrics: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    const hipStream_t st = (hipStream_t)stream;
    const int chunks = chunks_of(H, W);
    SSM_LAUNCH(flow_epe_kernel, dim3(chunks, N), dim3(FL_THREADS), 0, st, flow, gt_hw2, H * W, W, top, left, mode, (double *)workspace);
    SSM_LAUNCH(flow_epe_finish, dim3(N), dim3(FL_THREADS), 0, st, (const double *)workspace, chunks, out);
    return ssm::check_launch("ssm_flow_metrics_fwd");
}

extern "C" size_t ssm_flow_to_rgb_workspace_bytes(int N, int H, int W) {
    if (N < 1 || H < 1 || W < 1) return 0;
    return (size_t)N * chunks_of(H, W) * sizeof(float);
}

extern "C" int ssm_flow_to_rgb_fwd(ssm_view flow, unsigned char *rgb_hwc, int N, int H, int W, int top, int left, void *workspace,
                                   size_t workspace_bytes, void *stream) {
    SSM_REQUIRE(rgb_hwc && workspace, "flow_to_rgb: null pointer");
    if (int rc = check_field("flow_to_rgb", flow, N, H, W, top, left)) return rc;
    const size_t need = ssm_flow_to_rgb_workspace_bytes(N, H, W);
    SSM_REQUIRE(workspace_bytes >= need, "flow_to_rgb: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    const hipStream_t st = (hipStream_t)stream;
    const int chunks = chunks_of(H, W);
    SSM_LAUNCH(flow_maxrad_kernel, dim3(chunks, N), dim3(FL_THREADS), 0, st, flow, H * W, W, top, left, (float *)workspace);
    SSM_LAUNCH(flow_rgb_kernel, dim3(chunks, N), dim3(FL_THREADS), 0, st, flow, H * W, W, top, left, (const float *)workspace, rgb_hwc);
    return ssm::check_launch("ssm_flow_to_rgb_fwd");
}

extern "C" size_t ssm_flow_consistency_workspace_bytes(int N, int H, int W) {
    if (N < 1 || H < 1 || W < 1) return 0;
    return (size_t)N * chunks_of(H, W) * FC_WORDS * sizeof(unsigned long long);
}

extern "C" int ssm_flow_consistency_fwd(ssm_view flow4, int N, int H, int W, int top, int left, float alpha, float beta, void *workspace,
                                        double *out, unsigned char *mask, void *stream) {
    SSM_REQUIRE(workspace && out, "flow_consistency: null pointer");
    if (int rc = check_field("flow_consistency", flow4, N, H, W, top, left)) return rc;
    SSM_REQUIRE((reinterpret_cast<size_t>(workspace) & 7) == 0 && (reinterpret_cast<size_t>(out) & 7) == 0,
                "flow_consistency: workspace and out must be 8-byte aligned");
    const hipStream_t st = (hipStream_t)stream;
    const int chunks = chunks_of(H, W);
    SSM_LAUNCH(flow_consistency_kernel, dim3(chunks, N), dim3(FL_THREADS), 0, st, flow4, H * W, H, W, top, left, alpha, beta,
               (unsigned long long *)workspace, mask);
    SSM_LAUNCH(flow_consistency_finish, dim3(N), dim3(FL_THREADS), 0, st, (const unsigned long long *)workspace, chunks, out);
    return ssm::check_launch("ssm_flow_consistency_fwd");
}
