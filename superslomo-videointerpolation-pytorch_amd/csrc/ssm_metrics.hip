// Per-frame quality-metric sums of the evaluator (scripts/evaluate_interpolation_results.py:101-108: skimage's
// peak_signal_noise_ratio, structural_similarity(..., multichannel=True, gaussian_weights=True) and the interpolation error) on
// uint8 HWC frame stacks, in two deterministic launches:
//   metrics_tile_kernel    one 32x16 output tile of one frame per workgroup: the halo tile of both frames in LDS (scipy's
//                          mode="reflect" addressing), the separable 11-tap Gaussian of x, y, x*x, y*y, x*y per channel in fp64
//                          (horizontal pass into LDS, vertical pass in registers), the SSIM map, and a fixed-order workgroup sum of
//                          (SSE, IE, SSIM c0, c1, c2) into the tile's own slot of the caller's workspace;
//   metrics_finish_kernel  one workgroup per frame: the frame's slots summed in a fixed order into out[n][5].
// No atomics: the bits depend only on the frame's pixels and size, not on N or on the run.  fp64 because the cancellation in
// E[x^2] - E[x]^2 (~6.5e4 against C2 = 58.5) leaves too few bits in fp32.  The SSE is a sum of integers below 2^53: exact.
#include "ssm_common.h"

#include <cmath>

namespace {

constexpr int MT_W = 32, MT_H = 16;              // output tile
constexpr int MT_R = 5;                          // Gaussian radius: int(truncate 3.5 * sigma 1.5 + 0.5)
constexpr int MT_TAPS = 2 * MT_R + 1;
constexpr int MT_HW = MT_W + 2 * MT_R, MT_HH = MT_H + 2 * MT_R;      // halo tile 42 x 26
constexpr int MT_THREADS = 256;
constexpr int MT_ROWS = MT_H * MT_W / MT_THREADS;                     // output rows per thread (2)
static_assert(MT_W == 32 && MT_THREADS % MT_W == 0 && MT_H * MT_W == MT_ROWS * MT_THREADS, "tile shape");

struct GaussTaps {
    double w[MT_TAPS];
};

// scipy.ndimage mode="reflect" (d c b a | a b c d | d c b a), then clamped into the frame.  No output that is summed reads a reflected
// position: an interior output [5,H-5) x [5,W-5) reads rows 0..H-1 and columns 0..W-1 only.  The reflection gives the border outputs
// of the SSIM map scipy's values (they are masked out of the sums); the clamp keeps every read of a ragged tile inside the frame.
__device__ __forceinline__ int reflect_clamp(int i, int n) {
    if (i < 0) i = -1 - i;
    if (i >= n) i = 2 * n - 1 - i;
    return i < 0 ? 0 : (i >= n ? n - 1 : i);
}

__global__ __launch_bounds__(MT_THREADS) void metrics_tile_kernel(const unsigned char *__restrict__ tgt, const unsigned char *__restrict__ out,
                                                                  int H, int W, GaussTaps g, double *__restrict__ ws) {
    __shared__ __attribute__((aligned(16))) double hs[5][MT_HH][MT_W];          // horizontal pass: sx, sy, sxx, syy, sxy
    __shared__ __attribute__((aligned(16))) double red[5][MT_THREADS];
    __shared__ unsigned char raw[2][3][MT_HH][MT_HW];                           // halo tile of both frames, channel planes
    const int tid = threadIdx.x, n = blockIdx.z;
    const int tx0 = blockIdx.x * MT_W, ty0 = blockIdx.y * MT_H;
    const size_t frame = (size_t)n * H * W * 3;

    for (int i = tid; i < MT_HH * MT_HW * 3; i += MT_THREADS) {
        const int r = i / (MT_HW * 3), k = i - r * (MT_HW * 3), col = k / 3, c = k - col * 3;
        const size_t off = frame + ((size_t)reflect_clamp(ty0 - MT_R + r, H) * W + reflect_clamp(tx0 - MT_R + col, W)) * 3 + c;
        raw[0][c][r][col] = tgt[off];
        raw[1][c][r][col] = out[off];
    }
    __syncthreads();

    double w[MT_TAPS];
#pragma unroll
    for (int k = 0; k < MT_TAPS; ++k) w[k] = g.w[k];
    const int j = tid % MT_W, r0 = (tid / MT_W) * MT_ROWS;

    // SSE and IE of the thread's pixels
    double sse = 0.0, ie = 0.0;
#pragma unroll
    for (int q = 0; q < MT_ROWS; ++q) {
        int s2 = 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int d = (int)raw[0][c][r0 + q + MT_R][j + MT_R] - (int)raw[1][c][r0 + q + MT_R][j + MT_R];
            s2 += d * d;
        }
        if (ty0 + r0 + q < H && tx0 + j < W) {
            sse += (double)s2;
            ie += sqrt((double)s2);
        }
    }

    const double cov_norm = (double)(MT_TAPS * MT_TAPS) / (double)(MT_TAPS * MT_TAPS - 1);
    const double C1 = (0.01 * 255.0) * (0.01 * 255.0), C2 = (0.03 * 255.0) * (0.03 * 255.0);
    double ssim[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        for (int it = tid; it < MT_HH * MT_W; it += MT_THREADS) {
            const int r = it / MT_W, jj = it % MT_W;
            double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
#pragma unroll
            for (int k = 0; k < MT_TAPS; ++k) {
                const int x = raw[0][c][r][jj + k], y = raw[1][c][r][jj + k];
                sx = fma(w[k], (double)x, sx);
                sy = fma(w[k], (double)y, sy);
                sxx = fma(w[k], (double)(x * x), sxx);
                syy = fma(w[k], (double)(y * y), syy);
                sxy = fma(w[k], (double)(x * y), sxy);
            }
            hs[0][r][jj] = sx;
            hs[1][r][jj] = sy;
            hs[2][r][jj] = sxx;
            hs[3][r][jj] = syy;
            hs[4][r][jj] = sxy;
        }
        __syncthreads();
        double acc[MT_ROWS][5];
#pragma unroll
        for (int q = 0; q < MT_ROWS; ++q)
#pragma unroll
            for (int m = 0; m < 5; ++m) acc[q][m] = 0.0;
#pragma unroll
        for (int rr = 0; rr < MT_ROWS - 1 + MT_TAPS; ++rr) {
            double v[5];
#pragma unroll
            for (int m = 0; m < 5; ++m) v[m] = hs[m][r0 + rr][j];
#pragma unroll
            for (int q = 0; q < MT_ROWS; ++q) {
                const int k = rr - q;
                if (k >= 0 && k < MT_TAPS) {
#pragma unroll
                    for (int m = 0; m < 5; ++m) acc[q][m] = fma(w[k], v[m], acc[q][m]);
                }
            }
        }
        ssim[c] = 0.0;
#pragma unroll
        for (int q = 0; q < MT_ROWS; ++q) {
            const double ux = acc[q][0], uy = acc[q][1];
            const double vx = cov_norm * (acc[q][2] - ux * ux), vy = cov_norm * (acc[q][3] - uy * uy);
            const double vxy = cov_norm * (acc[q][4] - ux * uy);
            const double s = ((2.0 * ux * uy + C1) * (2.0 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2));
            const int oy = ty0 + r0 + q, ox = tx0 + j;
            if (oy >= MT_R && oy < H - MT_R && ox >= MT_R && ox < W - MT_R) ssim[c] += s;
        }
        __syncthreads();          // hs is rewritten by the next channel
    }

    red[0][tid] = sse;
    red[1][tid] = ie;
    red[2][tid] = ssim[0];
    red[3][tid] = ssim[1];
    red[4][tid] = ssim[2];
    __syncthreads();
    for (int s = MT_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) {
#pragma unroll
            for (int m = 0; m < 5; ++m) red[m][tid] += red[m][tid + s];
        }
        __syncthreads();
    }
    if (tid < 5) ws[(((size_t)n * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 5 + tid] = red[tid][0];
}

__global__ __launch_bounds__(MT_THREADS) void metrics_finish_kernel(const double *__restrict__ ws, int tiles, double *__restrict__ out) {
    __shared__ double red[5][MT_THREADS];
    const int tid = threadIdx.x, n = blockIdx.x;
    double a[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int t = tid; t < tiles; t += MT_THREADS) {
#pragma unroll
        for (int m = 0; m < 5; ++m) a[m] += ws[((size_t)n * tiles + t) * 5 + m];
    }
#pragma unroll
    for (int m = 0; m < 5; ++m) red[m][tid] = a[m];
    __syncthreads();
    for (int s = MT_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) {
#pragma unroll
            for (int m = 0; m < 5; ++m) red[m][tid] += red[m][tid + s];
        }
        __syncthreads();
    }
    if (tid < 5) out[(size_t)n * 5 + tid] = red[tid][0];
}

inline int tiles_x(int W) { return (W + MT_W - 1) / MT_W; }
inline int tiles_y(int H) { return (H + MT_H - 1) / MT_H; }

// scipy.ndimage._filters._gaussian_kernel1d(sigma=1.5, order=0, radius=5) in double: exp(-0.5 / sigma^2 * x^2) over x = -5..5,
// divided by its sum, the sum taken in numpy's order for 11 items (eight partial sums combined pairwise, then the last three).
GaussTaps gaussian_taps() {
    const double sigma = 1.5, a = -0.5 / (sigma * sigma);
    GaussTaps g;
    for (int k = 0; k < MT_TAPS; ++k) g.w[k] = std::exp(a * (double)((k - MT_R) * (k - MT_R)));
    const double *p = g.w;
    double sum = ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]));
    for (int k = 8; k < MT_TAPS; ++k) sum += p[k];
    for (int k = 0; k < MT_TAPS; ++k) g.w[k] /= sum;
    return g;
}

}  // namespace

extern "C" size_t ssm_frame_metrics_workspace_bytes(int N, int H, int W) {
    if (N < 1 || H < 1 || W < 1) return 0;
    return (size_t)N * tiles_x(W) * tiles_y(H) * 5 * sizeof(double);
}

extern "C" int ssm_frame_metrics_fwd(const unsigned char *target_hwc, const unsigned char *output_hwc, int N, int H, int W, void *workspace,
                                     size_t workspace_bytes, double *out, void *stream) {
    SSM_REQUIRE(target_hwc && output_hwc && workspace && out, "frame_metrics: null pointer");
    SSM_REQUIRE(N >= 1 && N <= 65535, "frame_metrics: N = %d outside [1, 65535]", N);
    SSM_REQUIRE(H >= MT_TAPS && W >= MT_TAPS, "frame_metrics: %dx%d frame is smaller than the 11x11 SSIM window", H, W);
    SSM_REQUIRE(tiles_y(H) <= 65535 && (long long)H * W * 3 < (1LL << 40), "frame_metrics: %dx%d frame too large", H, W);
    const size_t need = ssm_frame_metrics_workspace_bytes(N, H, W);
    SSM_REQUIRE(workspace_bytes >= need, "frame_metrics: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    const hipStream_t st = (hipStream_t)stream;
    SSM_LAUNCH(metrics_tile_kernel, dim3(tiles_x(W), tiles_y(H), N), dim3(MT_THREADS), 0, st, target_hwc, output_hwc, H, W, gaussian_taps(),
               (double *)workspace);
    SSM_LAUNCH(metrics_finish_kernel, dim3(N), dim3(MT_THREADS), 0, st, (const double *)workspace, tiles_x(W) * tiles_y(H), out);
    return ssm::check_launch("ssm_frame_metrics_fwd");
}
