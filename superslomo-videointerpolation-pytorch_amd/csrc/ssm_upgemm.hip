// The decoder step conv3x3(upsample2x(cat[a, b])) (scripts/models/flow_computation.py:244-247) as a 1x1 GEMM at LOW resolution followed by
// the nine filter taps applied after the upsample.
//
// Bilinear upsampling acts on every channel alone, the channel mixing of one filter tap is a matrix, and the two commute:
//
//   conv3x3(up(x))(Y, X) = bias + sum_{u,v in 0..2} [ (Y+u-1, X+v-1) inside the hi-res map ] * up(y_uv)(Y+u-1, X+v-1)
//   y_uv = W[:, :, u, v] . x          (a 1x1 convolution of the LOW-res input, Cin -> Cout, one per tap)
//
// with `up` ATen's half-pixel rule (edge-clamped source indices) and the bracket the convolution's zero padding.  The layer is one
// plain GEMM Cin -> 9 Cout on a quarter of the pixels - 9/36 of the direct form's multiply-adds, what F(4x4,3x3) issues too, but with
// no input transform, no output transform, no LDS expander and no Winograd filter transform around the matrix loop - and a cheap
// memory-bound pass that gathers the nine shifted bilinear samples.
//
//   upgemm_kernel          Y[b][tap Cout + co][y][x] = sum_ci Wp[tap Cout + co][ci] X[b][ci][y][x]   fp32 MFMA (v_mfma_f32_32x32x2_f32),
//                          raw sums into a scratch set of planes (interiors only); operands by LDS-DMA, double-buffered, one barrier
//                          per chunk of CK input channels (the structure of conv_mfma_kernel, csrc/ssm_conv.hip, without taps / halo)
//   upgemm_combine_kernel  out = LeakyReLU(bias + addend + the nine shifted bilinear gathers of Y)   one thread per 2 x 8 outputs
//   upgemm_pack_kernel     OIHW filter -> [9 Cout / 128][CinP][128] slabs of the GEMM's A operand
#include "ssm_conv_host.h"
#include "ssm_device.h"

#include <atomic>
#include <cstdlib>

namespace {

constexpr int BM = 128;      // GEMM rows (tap, cout) per workgroup
constexpr int CK = 16;       // input channels per chunk (one barrier per chunk: 8 k-steps of 8 / 4 MFMAs per wave)

struct GemmParams {
    const float *src1;
    const float *src2;
    long long sb1, sb2;      // batch strides (sb2 = 0: the second source is batch-broadcast)
    long long sc;            // channel stride (both sources)
    int sh;                  // row stride (both sources)
    int C1, Cin, CinP;       // channels of source 1, total, total rounded up to CK
    const float *wpk;
    float *dst;              // scratch planes [B][M][h][.]
    long long dsb, dsc;
    int dsh;
    int h, w, M;             // low-res map, GEMM rows = 9 Cout
    int tilesX, tilesY, NB;
};

// A workgroup = 4 waves as 2 (row halves of BM) x 2 (pixel rows); a wave owns 2 x MT accumulator tiles of 32 rows x 32 pixels, a
// 32-pixel group being 4 rows x 8 columns (the low-res maps are 40 / 80 / 160 wide: whole groups).
template <int MTY_, int MTX_>
struct GCfg {
    static constexpr int MTY = MTY_, MTX = MTX_, MT = MTY_ * MTX_, NT = 2, WN = 2, WY = 2;
    static constexpr int GW = 8, GH = 4;
    static constexpr int TH = MTY * GH * WY, TW = MTX * GW;
    static constexpr int TW4 = TW / 4;
    static constexpr int WSZ = CK * BM, PSZ = CK * TH * TW;
    static constexpr int NWQ = WSZ / 4, NDQ = PSZ / 4, NQ = NWQ + NDQ;          // 16-byte pieces per chunk
    static constexpr int NG = NQ / 64, NI = NG / 4;                              // 1-KiB wave-instructions per chunk, per wave
    static constexpr int STAGE = WSZ + PSZ;
    static constexpr int BYTES = 2 * STAGE * 4;
    static_assert(TW == 16, "the patch swizzle below is written for 16-float rows");
    static_assert(NWQ % 64 == 0 && NQ % 256 == 0, "every wave-instruction is all filter or all patch; equal shares per wave");
    static_assert(BYTES <= 65536, "LDS budget (two workgroups per CU)");
};

// Patch rows are 16 floats.  Row r keeps its two 8-float halves swapped when bit 1 of r is set, so the four rows of a 4 x 8 pixel group
// sit on 32 distinct banks (rows 0 / 2 would share theirs): LDS-DMA writes linearly, so the SOURCE piece index carries the swap, and
// the reader applies the same involution.
__device__ __forceinline__ int swz_piece(int r, int j) { return j ^ (((r >> 1) & 1) << 1); }

// RAGGED: the sources' channel counts are no multiples of CK - a chunk may straddle the two sources or run past Cin (those
// channels' filter entries are zero; their activations are fetched from channel 0, which is finite).  Per-lane 64-bit addresses.
template <class C, bool RAGGED>
__global__ __launch_bounds__(256, 2) void upgemm_kernel(const GemmParams p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int NT = C::NT, MT = C::MT, GW = C::GW, GH = C::GH, TH = C::TH, TW = C::TW;

    const int tid = threadIdx.x;
    const int lane = tid & 63, l31 = lane & 31, half = lane >> 5;
    const int gy = l31 / GW, gx = l31 % GW;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wn = wid % C::WN, wy = wid / C::WN;

    int id = ssm_xcd_tile(blockIdx.x, gridDim.x);
    const int nb = id % p.NB;
    id /= p.NB;
    const int tx = id % p.tilesX;
    id /= p.tilesX;
    const int ty = id % p.tilesY;
    const int b = id / p.tilesY;
    const int x0 = tx * TW, y0 = ty * TH;
    const int nchunks = p.CinP / CK;

    const long long porg = (long long)y0 * p.sh + x0;
    const float *pbase1 = p.src1 + (long long)b * p.sb1 + porg;
    const float *pbase2 = p.src2 + (long long)b * p.sb2 + porg;
    const float *wbase = p.wpk + (long long)nb * p.CinP * BM;

    // per-lane source offset of each LDS-DMA piece this wave issues (same for every chunk); wave-instruction g = 4 k + wave
    int off[C::NI];
    int pch[C::NI];          // RAGGED: the piece's channel inside the chunk
#pragma unroll
    for (int i = 0; i < C::NI; ++i) {
        const int q = (i * 4 + wid) * 64 + lane;
        if (q < C::NWQ) {
            off[i] = q * 4;
            pch[i] = 0;
        } else {
            const int qq = q - C::NWQ;
            const int c = qq / (TH * C::TW4);
            const int rem = qq - c * (TH * C::TW4);
            const int r = rem / C::TW4, j = swz_piece(r, rem % C::TW4);
            pch[i] = c;
            off[i] = (RAGGED ? 0 : (int)(c * p.sc)) + r * p.sh + 4 * j;
        }
    }
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) void *)lds;
    auto issue_k = [&](int ch, int stage, int k) {
        const int c0 = ch * CK;
        const float *wb = wbase + (long long)c0 * BM;
        const unsigned lsb = lds0 + (unsigned)(stage * C::STAGE) * 4u;
#pragma unroll
        for (int wv = 0; wv < 4; ++wv) {
            const int g = 4 * k + wv;
            if (wv == wid) {          // wave-uniform
                const bool is_w = g * 64 < C::NWQ;
                if (is_w) {
                    lds_dma16(wb, off[k] * 4, lsb + (unsigned)g * 1024u);
                } else if constexpr (!RAGGED) {
                    const float *pb = (c0 < p.C1) ? pbase1 + (long long)c0 * p.sc : pbase2 + (long long)(c0 - p.C1) * p.sc;
                    lds_dma16(pb, off[k] * 4, lsb + (unsigned)g * 1024u);
                } else {
                    const int cg = c0 + pch[k];
                    const float *pb = cg < p.C1 ? pbase1 + (long long)cg * p.sc : (cg < p.Cin ? pbase2 + (long long)(cg - p.C1) * p.sc : pbase1);
                    SSM_GLDS16(pb + off[k], lds + stage * C::STAGE + g * 256);
                }
            }
        }
    };

    f32x16 acc[NT][MT];
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[n][m][r] = 0.f;

    // per-lane operand bases (floats): filter inside a stage; activation inside the patch, one base per column group (the swizzle)
    const int aBase = half * BM + wn * (NT * 32) + l31;
    const int sw = ((gy >> 1) & 1) * 8;
    int bBase[C::MTX];
#pragma unroll
    for (int mx = 0; mx < C::MTX; ++mx) bBase[mx] = C::WSZ + half * (TH * TW) + (wy * C::MTY * GH + gy) * TW + ((mx * GW) ^ sw) + gx;

#pragma unroll
    for (int k = 0; k < C::NI; ++k) issue_k(0, 0, k);
    for (int ch = 0; ch < nchunks; ++ch) {
        // chunk ch has landed for every wave; every wave is done reading chunk ch-1
        wait_vmcnt<0>();
        __syncthreads();
        const bool dma_next = ch + 1 < nchunks;
        const float *stg = lds + (ch & 1) * C::STAGE;
        // operand fetches one k-step ahead in a second register set, the next chunk's DMA one instruction per k-step behind the first MFMA
        // (conv_mfma_kernel's schedule)
        constexpr int S = CK / 2;
        float a[2][NT], bv[2][MT];
        auto fetch = [&](int s, int buf) {
#pragma unroll
            for (int n = 0; n < NT; ++n) a[buf][n] = stg[aBase + 2 * s * BM + n * 32];
#pragma unroll
            for (int my = 0; my < C::MTY; ++my)
#pragma unroll
                for (int mx = 0; mx < C::MTX; ++mx) bv[buf][my * C::MTX + mx] = stg[bBase[mx] + (2 * s * TH + my * GH) * TW];
        };
        fetch(0, 0);
#pragma unroll
        for (int s = 0; s < S; ++s) {
#pragma unroll
            for (int n = 0; n < NT; ++n)
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    acc[n][m] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s & 1][n], bv[s & 1][m], acc[n][m], 0, 0, 0);
                    if (n == 0 && m == 0) {
                        __builtin_amdgcn_sched_barrier(0);
                        if (s + 1 < S) fetch(s + 1, (s + 1) & 1);
                        if (s < C::NI && dma_next) issue_k(ch + 1, (ch + 1) & 1, s);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            __builtin_amdgcn_sched_barrier(0);
        }
        static_assert(C::NI <= S, "one DMA instruction per k-step");
    }

    // ---- store the raw sums: register r of lane (l31, half) = row (r&3) + 8*(r>>2) + 4*half of the 32-row block, pixel l31 of the group
    const int xbase = x0 + gx, ybase = y0 + wy * (C::MTY * GH) + gy;
    float *dstb = p.dst + (long long)b * p.dsb;
    const int m0 = nb * BM + wn * (NT * 32);          // first GEMM row of this wave (uniform)
    const unsigned pbase = 4u * ((unsigned)(4 * half) * (unsigned)p.dsc + (unsigned)ybase * (unsigned)p.dsh + (unsigned)xbase);
    bool pok[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) pok[m] = ybase + (m / C::MTX) * GH < p.h && xbase + (m % C::MTX) * GW < p.w;
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        if (m0 + n * 32 < p.M) {          // uniform; M is a multiple of 32: a 32-row block is whole or padding
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int mu = m0 + n * 32 + (r & 3) + 8 * (r >> 2);
                float *bp = dstb + (long long)mu * p.dsc;
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    float *bpm = bp + ((m / C::MTX) * GH) * p.dsh + (m % C::MTX) * GW;          // uniform
                    if (pok[m]) store_sbase(bpm, pbase, acc[n][m][r]);
                }
            }
        }
    }
}

using G16 = GCfg<2, 2>;      // 16 x 16 low-res pixels per workgroup
using G8 = GCfg<1, 2>;       //  8 x 16: maps whose height a 16-row tile overshoots by much (23 x 40)
enum GemmKind { KG16, KG8, NGKIND };
constexpr int kTH[NGKIND] = {G16::TH, G8::TH}, kTW[NGKIND] = {G16::TW, G8::TW};

ssm::ForcedKind g_force_kind;          // tests / tuning only (ssm_upgemm_force_kind)

int pick_kind(int h, int w) {
    const int forced = g_force_kind.get(NGKIND);
    if (forced >= 0) return forced;
    long long best = 0;
    int kd = 0;
    for (int i = 0; i < NGKIND; ++i) {          // fewest computed pixels; the larger tile on a tie
        const long long px = (long long)((h + kTH[i] - 1) / kTH[i]) * kTH[i] * ((w + kTW[i] - 1) / kTW[i]) * kTW[i];
        if (i == 0 || px < best) {
            best = px;
            kd = i;
        }
    }
    return kd;
}

template <class C>
int launch_gemm(GemmParams &p, int B, bool ragged, hipStream_t st) {
    p.tilesX = (p.w + C::TW - 1) / C::TW;
    p.tilesY = (p.h + C::TH - 1) / C::TH;
    const long long blocks = (long long)p.tilesX * p.tilesY * p.NB * B;
    SSM_TRY(ssm::check_grid("upgemm", blocks));
    if (ragged) SSM_LAUNCH((upgemm_kernel<C, true>), dim3((unsigned)blocks), dim3(256), C::BYTES, st, p);
    else SSM_LAUNCH((upgemm_kernel<C, false>), dim3((unsigned)blocks), dim3(256), C::BYTES, st, p);
    return ssm::check_launch("ssm_upgemm_conv2d_ups_add_fwd (gemm)");
}

// ---- the taps after the upsample --------------------------------------------------------------------------------------------------
struct CombineParams {
    const float *y;          // scratch planes [B][9 Cout][h][.]
    long long ysb, ysc;
    int ysh;
    const float *bias;
    float *dst;
    long long dsb, dsc;
    int dsh;
    const float *add;        // optional pre-activation addend [B / adiv][Cout][H][W]
    long long asb, asc;
    int ash, adiv;
    int h, w, Cout, nq;      // low-res map; quads (4 low-res columns) per row
    long long total;         // threads: B Cout h nq
    float slope;
};

// One thread = low-res row i, columns j0 .. j0+3 of one output channel = hi-res rows 2i, 2i+1, columns 2 j0 .. 2 j0 + 7.  Per tap
// column v the three tap rows u are combined along y first - V[dy][c] over the six low-res columns j0-1 .. j0+4, from 2 / 3 / 2 rows of
// the planes (u, v) with the half-pixel weights 1/4, 3/4 (source rows clamped at the edge, weight zero where the tap's hi-res row lies
// outside the map) - then interpolated along x at the eight hi-res columns the tap reads (zero outside the map).  The products of the two
// passes are the nine taps x four corners weights 1/16, 3/16, 9/16.  W4: w is a multiple of 4 - a quad is whole: one 16-byte load per row.
template <bool W4>
__global__ __launch_bounds__(256) void upgemm_combine_kernel(const CombineParams p) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= p.total) return;
    long long r = t;
    const int q = (int)(r % p.nq);
    r /= p.nq;
    const int i = (int)(r % p.h);
    r /= p.h;
    const int co = (int)(r % p.Cout);
    const int b = (int)(r / p.Cout);
    const int j0 = 4 * q;
    const int W = 2 * p.w;

    const int rowm = max(i - 1, 0), rowp = min(i + 1, p.h - 1);
    const int cm = max(j0 - 1, 0), cp = min(j0 + 4, p.w - 1);
    const float mt = i > 0 ? 1.f : 0.f, mb = i < p.h - 1 ? 1.f : 0.f;          // hi-res rows 2i - 1 / 2i + 2 inside the map
    const float *yb = p.y + (long long)b * p.ysb + (long long)co * p.ysc;
    const long long tapc = (long long)p.Cout * p.ysc;

    float acc[2][8];
#pragma unroll
    for (int d = 0; d < 2; ++d)
#pragma unroll
        for (int x = 0; x < 8; ++x) acc[d][x] = 0.f;

    auto load_row = [&](const float *plane, int row, float (&c)[6]) {
        const float *rp = plane + (long long)row * p.ysh;
        c[0] = rp[cm];
        if constexpr (W4) {
            const f32x4 v = *(const f32x4 *)(rp + j0);
            c[1] = v[0], c[2] = v[1], c[3] = v[2], c[4] = v[3];
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) c[1 + k] = rp[min(j0 + k, p.w - 1)];
        }
        c[5] = rp[cp];
    };
#pragma unroll
    for (int v = 0; v < 3; ++v) {
        float V[2][6];
        float c[6];
        // u = 0: hi-res rows 2i-1 (dy 0) and 2i (dy 1) from low rows i-1, i
        const float *pl = yb + (long long)v * tapc;
        load_row(pl, rowm, c);
#pragma unroll
        for (int k = 0; k < 6; ++k) V[0][k] = (0.75f * mt) * c[k], V[1][k] = 0.25f * c[k];
        load_row(pl, i, c);
#pragma unroll
        for (int k = 0; k < 6; ++k) V[0][k] += (0.25f * mt) * c[k], V[1][k] += 0.75f * c[k];
        // u = 1: rows 2i (dy 0: low i-1, i) and 2i+1 (dy 1: low i, i+1)
        pl = yb + (long long)(3 + v) * tapc;
        load_row(pl, rowm, c);
#pragma unroll
        for (int k = 0; k < 6; ++k) V[0][k] += 0.25f * c[k];
        load_row(pl, i, c);
#pragma unroll
        for (int k = 0; k < 6; ++k) V[0][k] += 0.75f * c[k], V[1][k] += 0.75f * c[k];
        load_row(pl, rowp, c);
#pragma unroll
        for (int k = 0; k < 6; ++k) V[1][k] += 0.25f * c[k];
        // u = 2: rows 2i+1 (dy 0) and 2i+2 (dy 1) from low rows i, i+1
        pl = yb + (long long)(6 + v) * tapc;
        load_row(pl, i, c);
#pragma unroll
        for (int k = 0; k < 6; ++k) V[0][k] += 0.75f * c[k], V[1][k] += (0.25f * mb) * c[k];
        load_row(pl, rowp, c);
#pragma unroll
        for (int k = 0; k < 6; ++k) V[0][k] += 0.25f * c[k], V[1][k] += (0.75f * mb) * c[k];
        // along x: output column 2 j0 + x reads hi-res column Q = 2 j0 + x + v - 1 = 2 j0 + tt; V index 0 = low column j0 - 1
#pragma unroll
        for (int x = 0; x < 8; ++x) {
            const int tt = x + v - 1;
            const int k = (tt + 2) / 2 - 1;          // floor(tt / 2) for tt >= -1
            const bool odd = (tt & 1) != 0;
            const int ia = odd ? k + 1 : k, ib = ia + 1;
            const float wa = odd ? 0.75f : 0.25f, wb = odd ? 0.25f : 0.75f;
            const int Q = 2 * j0 + tt;
            const bool in = Q >= 0 && Q < W;
#pragma unroll
            for (int d = 0; d < 2; ++d) {
                const float u = wa * V[d][ia] + wb * V[d][ib];
                acc[d][x] += in ? u : 0.f;
            }
        }
    }
    const float bs = p.bias[co];
    const float sl = p.slope;
    float *dp = p.dst + (long long)b * p.dsb + (long long)co * p.dsc + (long long)(2 * i) * p.dsh + 2 * j0;
    const float *ap = p.add ? p.add + (long long)(b / p.adiv) * p.asb + (long long)co * p.asc + (long long)(2 * i) * p.ash + 2 * j0 : nullptr;
    const int nx = min(8, W - 2 * j0);          // (even)
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        float o[8];
#pragma unroll
        for (int x = 0; x < 8; ++x) o[x] = acc[d][x] + bs;
        if (ap) {
            const float *a = ap + (long long)d * p.ash;
            if (W4 || nx == 8) {
                const f32x4 a0 = *(const f32x4 *)a, a1 = *(const f32x4 *)(a + 4);
#pragma unroll
                for (int x = 0; x < 4; ++x) o[x] += a0[x], o[4 + x] += a1[x];
            } else {
#pragma unroll
                for (int x = 0; x < 8; ++x)
                    if (x < nx) o[x] += a[x];
            }
        }
#pragma unroll
        for (int x = 0; x < 8; ++x) o[x] = fmaxf(o[x], o[x] * sl);
        float *dr = dp + (long long)d * p.dsh;
        if (W4 || nx == 8) {
            f32x4 s0, s1;
#pragma unroll
            for (int x = 0; x < 4; ++x) s0[x] = o[x], s1[x] = o[4 + x];
            *(f32x4 *)dr = s0;
            *(f32x4 *)(dr + 4) = s1;
        } else {
#pragma unroll
            for (int x = 0; x < 8; ++x)
                if (x < nx) dr[x] = o[x];
        }
    }
}

__global__ void upgemm_pack_kernel(const float *__restrict__ w, float *__restrict__ wp, int Cout, int Cin, int CinP, long long total) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    // packed index -> (row block, cin, row in block); GEMM row m = tap Cout + cout
    const int n = (int)(i % BM);
    const long long r = i / BM;
    const int ci = (int)(r % CinP);
    const int m = (int)(r / CinP) * BM + n;
    float v = 0.f;
    if (m < 9 * Cout && ci < Cin) {
        const int tap = m / Cout, co = m - tap * Cout;
        v = w[((long long)co * Cin + ci) * 9 + tap];
    }
    wp[i] = v;
}

inline int round_up(int a, int b) { return (a + b - 1) / b * b; }

}  // namespace

extern "C" int ssm_upgemm_supported(int Cin, int Cout, int H, int W, int k) {
    return k == 3 && Cin > 0 && Cout > 0 && Cout % 32 == 0 && H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0;
}

// The selection rule, from the per-layer A/B against the layer's F(4x4,3x3) launch (profiles/upgemm_layers_ab.txt): a layer is
// selected where GEMM + combine won by more than the run-to-run spread of that measurement.  The 9 Cout-channel intermediate costs 3.25x
// the output's bytes, so the form pays where the GEMM is long beside it (many input channels per output pixel) and the launch fills the
// chip; the one small-launch win is the 1/32 -> 1/16 level, where the Winograd form's tiles leave most of it idle.  px = B h w low-res
// pixels; measured at px = 1.8 k ... 914 k (stage 1 at batch 2, stage 2 at batch 14, the 4K plan at batch 7):
//   Cout 512 (conv7a):  -34 % at 1.8 k px, a tie at 12.9 k, +0.5 % at 57 k     -> the small launches only
//   Cout 256 (conv8a):  +9 % at 7.4 k px, -16 % at 51.5 k, -11 % at 228 k      -> the large launches
//   Cout 128 (conv9a):  a tie at 29 k px, -2.5 % at 206 k, -5 % at 914 k       -> the large launches
//   Cout  64 (conv10a): +14 ... +17 % everywhere; conv11a (Cout 32) by the same reasoning - the intermediate grows, the GEMM does not
extern "C" int ssm_upgemm_preferred(int Cin, int Cout, int B, int h, int w) {
    if (!ssm_upgemm_supported(Cin, Cout, 2 * h, 2 * w, 3) || B <= 0) return 0;
    const long long px = (long long)B * h * w;
    if (Cin >= 512 && Cout >= 512) return px <= 4096;
    if (Cin >= 1024 && Cout >= 256) return px >= 32768;
    if (Cin >= 512 && Cout >= 128) return px >= 131072;
    return 0;
}

extern "C" int ssm_upgemm_force_kind(int kind) {
    return g_force_kind.set(kind, NGKIND);
}

extern "C" size_t ssm_upgemm_packed_weight_floats(int Cout, int Cin) {
    return (size_t)round_up(9 * Cout, BM) * (size_t)round_up(Cin, CK);
}

extern "C" int ssm_upgemm_pack_weights(const float *w_oihw, float *w_packed, int Cout, int Cin, void *stream) {
    SSM_REQUIRE(w_oihw && w_packed, "upgemm pack_weights: null pointer");
    SSM_REQUIRE(Cout > 0 && Cin > 0 && Cout % 32 == 0, "upgemm pack_weights: bad sizes (Cout = %d must be a multiple of 32)", Cout);
    const long long total = (long long)ssm_upgemm_packed_weight_floats(Cout, Cin);
    SSM_LAUNCH(upgemm_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w_oihw, w_packed, Cout, Cin,
               round_up(Cin, CK), total);
    return ssm::check_launch("ssm_upgemm_pack_weights");
}

// scratch planes [B][9 Cout][h][round_up(w, 4)]: ssm_view {ptr, 9 Cout h wr, h wr, wr}
extern "C" size_t ssm_upgemm_scratch_floats(int Cout, int B, int h, int w) {
    return (size_t)B * 9 * (size_t)Cout * (size_t)h * (size_t)round_up(w, 4);
}

extern "C" int ssm_upgemm_conv2d_ups_add_fwd(ssm_view a, int C1, ssm_view b, int C2, const float *w_packed, const float *bias, ssm_view scratch,
                                             ssm_view y, ssm_view add, int add_div, int B, int H, int W, int Cout, float slope, int flags,
                                             void *stream) {
    SSM_REQUIRE(B > 0 && C1 > 0 && C2 >= 0, "upgemm: bad batch / channel counts");
    SSM_REQUIRE(ssm_upgemm_supported(C1 + C2, Cout, H, W, 3), "upgemm: unsupported problem (Cout = %d must be a multiple of 32, H x W = %d x %d even)",
                Cout, H, W);
    SSM_REQUIRE(a.ptr && y.ptr && scratch.ptr && w_packed && bias, "upgemm: null pointer");
    const int h = H / 2, w = W / 2;
    SSM_REQUIRE(ssm::aligned16(a.ptr) && a.sh % 4 == 0 && a.sc % 4 == 0 && a.sb % 4 == 0, "upgemm: input 1 is not a padded-plane view (16-byte alignment)");
    SSM_REQUIRE(a.sh >= w + 2 * SSM_PADX, "upgemm: input 1 row stride %d leaves no frame for w=%d", a.sh, w);
    SSM_REQUIRE(ssm::aligned16(w_packed), "upgemm: packed filter must be 16-byte aligned");
    if (C2 > 0) {
        SSM_REQUIRE(b.ptr && ssm::aligned16(b.ptr) && b.sb % 4 == 0, "upgemm: input 2 is not a padded-plane view");
        SSM_REQUIRE(b.sh == a.sh && b.sc == a.sc, "upgemm: cat sources must share row/channel strides");
    }
    SSM_REQUIRE(4LL * ((long long)CK * a.sc + 32LL * a.sh) < 0x7fffffffLL, "upgemm: channel stride too large");
    SSM_REQUIRE(ssm::aligned16(scratch.ptr) && scratch.sh % 4 == 0 && scratch.sh >= w && scratch.sc % 4 == 0 && scratch.sb % 4 == 0 &&
                    scratch.sc >= (long long)h * scratch.sh && scratch.sb >= 9LL * Cout * scratch.sc,
                "upgemm: scratch view too small or misaligned for 9 x %d planes of %d x %d", Cout, h, w);
    SSM_REQUIRE(4LL * (4 * scratch.sc + (long long)(h + 32) * scratch.sh) < 0x7fffffffLL, "upgemm: scratch plane too large for 32-bit offsets");
    SSM_REQUIRE(ssm::aligned16(y.ptr) && y.sh % 4 == 0 && y.sc % 4 == 0 && y.sb % 4 == 0, "upgemm: output is not a padded-plane view (16-byte alignment)");
    if (add.ptr) {
        SSM_REQUIRE(add_div >= 1 && B % add_div == 0, "upgemm: the addend serves %d batch entries each, batch %d is no multiple", add_div, B);
        SSM_REQUIRE(ssm::aligned16(add.ptr) && add.sh % 4 == 0 && add.sc % 4 == 0 && add.sb % 4 == 0, "upgemm: addend is not a padded-plane view");
    }
    hipStream_t st = (hipStream_t)stream;

    GemmParams g;
    g.src1 = a.ptr;
    g.src2 = C2 > 0 ? b.ptr : a.ptr;
    g.sb1 = a.sb;
    g.sb2 = C2 > 0 ? b.sb : 0;
    g.sc = a.sc;
    g.sh = a.sh;
    g.C1 = C1;
    g.Cin = C1 + C2;
    g.CinP = round_up(C1 + C2, CK);
    g.wpk = w_packed;
    g.dst = scratch.ptr;
    g.dsb = scratch.sb;
    g.dsc = scratch.sc;
    g.dsh = scratch.sh;
    g.h = h;
    g.w = w;
    g.M = 9 * Cout;
    g.NB = (g.M + BM - 1) / BM;
    const bool ragged = C1 % CK != 0 || (C1 + C2) % CK != 0;
    const int kd = pick_kind(h, w);
    const int rc = kd == KG16 ? launch_gemm<G16>(g, B, ragged, st) : launch_gemm<G8>(g, B, ragged, st);
    if (rc != SSM_OK) return rc;

    CombineParams c;
    c.y = scratch.ptr;
    c.ysb = scratch.sb;
    c.ysc = scratch.sc;
    c.ysh = scratch.sh;
    c.bias = bias;
    c.dst = y.ptr;
    c.dsb = y.sb;
    c.dsc = y.sc;
    c.dsh = y.sh;
    c.add = add.ptr;
    c.asb = add.ptr ? add.sb : 0;
    c.asc = add.ptr ? add.sc : 0;
    c.ash = add.ptr ? add.sh : 0;
    c.adiv = add.ptr ? add_div : 1;
    c.h = h;
    c.w = w;
    c.Cout = Cout;
    c.nq = (w + 3) / 4;
    c.total = (long long)B * Cout * h * c.nq;
    c.slope = (flags & SSM_FLAG_LRELU) ? slope : 1.f;
    const long long blocks = (c.total + 255) / 256;
    SSM_REQUIRE(blocks > 0 && blocks <= 0x7fffffffLL, "upgemm: combine grid of %lld workgroups out of range", blocks);
    if (w % 4 == 0) SSM_LAUNCH(upgemm_combine_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, st, c);
    else SSM_LAUNCH(upgemm_combine_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, st, c);
    return ssm::check_launch("ssm_upgemm_conv2d_ups_add_fwd (combine)");
}
