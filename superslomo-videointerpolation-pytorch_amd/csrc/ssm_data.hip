// Training ingest: whole decoded uint8 HWC RGB frames in a staging buffer -> the cropped, augmented, normalised fp32 batch of the
// dataloader contract (ssm_amd/data.py), next to frames_from_u8_kernel of ssm_elem.hip, whose normalise expression it keeps.  One
// launch fuses the reference's RandomCrop, RandomMirrorRotate, Normalize and ToTensor (scripts/utils/dataloaders/default_reader.py:
// 182-207,250-286, augmentations.py:39-92,181-200) and the split of a sample's frames into the (input, target) tensors.
//   clip_batch_from_u8_kernel   one thread per four output pixels of a row, all three channels (rows and groups of four flattened into
//                               one index, so waves stay full at any crop width): a pure gather at one touch, 3 B read
//                               and 12 B written per output pixel; each channel's four floats go out as one 16-byte store when the
//                               planes allow it (tw % 4 == 0, aligned tensors), as scalar stores otherwise
// Source bytes sit at arbitrary alignment (x1 * 3 is arbitrary).  In integer mode on an untransposed frame a thread's four pixels are 12
// contiguous bytes: it loads the three or four ALIGNED dwords that cover them (lane i at 12 i: the wave reads 768 contiguous bytes) and
// shifts them into place; the buffer's base and size are multiples of 4 for that (checked by the launcher), so an aligned dword that
// holds one byte of the buffer lies inside it.  Everything else - a transposed frame (a column gather: portrait clips are rare), the
// row's tail, affine mode - reads single bytes.
// NO CONTRACTION (as ssm_video.hip): the numpy yardstick (ssm_amd.data.augment_host) rounds every operation, and so must the kernel.
#include "ssm_common.h"
#include "ssm_device.h"

#pragma clang fp contract(off)

namespace {

static_assert(sizeof(ssm_clip_record) == 64, "table record");

struct Norm3 {
    float m[3], s[3];
};

// byte address of channel 0 of logical pixel (ly, lx) of a stored Hs x Ws frame; the logical frame of a transposed one is its transpose
__device__ __forceinline__ const unsigned char *pixel(const unsigned char *frame, int Ws, bool transpose, int ly, int lx) {
    return frame + (transpose ? (long long)lx * Ws + ly : (long long)ly * Ws + lx) * 3;
}

__global__ __launch_bounds__(256) void clip_batch_from_u8_kernel(const unsigned char *__restrict__ frames, const ssm_clip_record *__restrict__ table,
                                                                 float *__restrict__ input, float *__restrict__ target, int F, int n_in, int th,
                                                                 int tw, Norm3 nm, int vec_in, int vec_out) {
    // (row, group of four pixels) flattened into one index: every wave but a frame's last is full whatever tw is
    const int qw = (tw + 3) >> 2;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= th * qw) return;
    const int y = idx / qw, x0 = 4 * (idx - y * qw);
    const int b = blockIdx.y / F, f = blockIdx.y - b * F;
    const ssm_clip_record *r = table + b;          // uniform in the workgroup
    const int Hs = r->hs, Ws = r->ws, flags = r->flags, y1 = r->y1, x1 = r->x1;
    const bool transpose = flags & SSM_CLIP_TRANSPOSE, hflip = flags & SSM_CLIP_HFLIP;
    const unsigned char *frame = frames + r->offset + (long long)f * Hs * Ws * 3;
    const bool whole = x0 + 3 < tw;
    float v[3][4];          // [channel][pixel]: the 8-bit values, or their bilinear sample
    if (flags & SSM_CLIP_AFFINE) {
        const float a00 = r->a[0], a01 = r->a[1], a02 = r->a[2], a10 = r->a[3], a11 = r->a[4], a12 = r->a[5];
        const float fy = (float)y;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float fx = (float)(x0 + j);
            const float u = (a00 * fx + a01 * fy) + a02, w = (a10 * fx + a11 * fy) + a12;          // position inside the (flipped) crop
            float s[3] = {0.0f, 0.0f, 0.0f};
            if (x0 + j < tw && u > -1.0f && u < (float)tw && w > -1.0f && w < (float)th) {          // else: every tap is outside (NaN too)
                const float uf = floorf(u), wf = floorf(w);
                const int cx = (int)uf, cy = (int)wf;          // -1 .. tw - 1, -1 .. th - 1
                const float ax = u - uf, ay = w - wf;
                const float bx = 1.0f - ax, by = 1.0f - ay;
                float p[2][2][3];
#pragma unroll
                for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                    for (int dx = 0; dx < 2; ++dx) {
                        const int ty = cy + dy, tx = cx + dx;
                        const bool in = ty >= 0 && ty < th && tx >= 0 && tx < tw;
                        const unsigned char *q = pixel(frame, Ws, transpose, y1 + (in ? ty : 0), x1 + (in ? (hflip ? tw - 1 - tx : tx) : 0));
#pragma unroll
                        for (int c = 0; c < 3; ++c) p[dy][dx][c] = in ? (float)q[c] : 0.0f;
                    }
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float top = p[0][0][c] * bx + p[0][1][c] * ax;
                    const float bot = p[1][0][c] * bx + p[1][1][c] * ax;
                    s[c] = top * by + bot * ay;
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c][j] = s[c];
        }
    } else if (vec_in && whole && !transpose) {
        // the thread's 12 source bytes: pixels x0 .. x0 + 3 of the crop row, or mirrored tw - 4 - x0 .. tw - 1 - x0, read back to front
        const unsigned char *p = pixel(frame, Ws, false, y1 + y, x1 + (hflip ? tw - 4 - x0 : x0));
        const unsigned sh = (unsigned)(reinterpret_cast<size_t>(p) & 3);
        const unsigned *a = reinterpret_cast<const unsigned *>(p - sh);
        const unsigned w0 = a[0], w1 = a[1], w2 = a[2], w3 = sh ? a[3] : 0u;
        const unsigned d[3] = {__builtin_amdgcn_alignbyte(w1, w0, sh), __builtin_amdgcn_alignbyte(w2, w1, sh),
                               __builtin_amdgcn_alignbyte(w3, w2, sh)};
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int k = 3 * j + c;          // byte k of the 12: pixel j of the run, channel c
                const float val = (float)((d[k >> 2] >> (8 * (k & 3))) & 255u);
                if (hflip) v[c][3 - j] = val;
                else v[c][j] = val;
            }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int x = min(x0 + j, tw - 1);
            const unsigned char *q = pixel(frame, Ws, transpose, y1 + y, x1 + (hflip ? tw - 1 - x : x));
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c][j] = (float)q[c];
        }
    }
    // frames 0 .. n_in - 1 of a sample are its inputs, the rest its targets
    const int nt = F - n_in;
    float *plane0 = f < n_in ? input + ((long long)b * n_in + f) * 3 * th * tw : target + ((long long)b * nt + (f - n_in)) * 3 * th * tw;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (v[c][j] / 255.0f - nm.m[c]) / nm.s[c];
        float *row = plane0 + ((long long)c * th + y) * tw + x0;
        if (vec_out && whole) {          // vec_out: tw % 4 == 0 and 16-byte aligned tensors
            f32x4 q;
            q.x = o[0], q.y = o[1], q.z = o[2], q.w = o[3];
            *reinterpret_cast<f32x4 *>(row) = q;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x0 + j < tw) row[j] = o[j];
        }
    }
}

}  // namespace

extern "C" int ssm_clip_batch_from_u8_fwd(const unsigned char *frames, long long frames_bytes, const ssm_clip_record *table_dev,
                                          const ssm_clip_record *table_host, float *input, float *target, int B, int F, int n_in, int th,
                                          int tw, const float *mean3, const float *std3, void *stream) {
    SSM_REQUIRE(frames && table_dev && table_host && input && target && mean3 && std3, "clip_batch_from_u8: null pointer");
    SSM_REQUIRE(B >= 1 && F >= 1 && th >= 1 && tw >= 1 && frames_bytes >= 1 && (long long)B * F <= 65535 &&
                    (long long)th * ((tw + 3) / 4) <= 0x7fffffffLL,
                "clip_batch_from_u8: bad geometry B %d, F %d, crop %dx%d, %lld bytes", B, F, th, tw, frames_bytes);
    SSM_REQUIRE(n_in >= 1 && n_in <= F - 1, "clip_batch_from_u8: n_in %d outside 1..F-1 = %d", n_in, F - 1);
    for (int b = 0; b < B; ++b) {
        const ssm_clip_record &r = table_host[b];
        SSM_REQUIRE(r.hs >= 1 && r.ws >= 1 && r.offset >= 0 && (r.flags & ~(SSM_CLIP_TRANSPOSE | SSM_CLIP_HFLIP | SSM_CLIP_AFFINE)) == 0,
                    "clip_batch_from_u8: sample %d: bad record (frame %dx%d, offset %lld, flags %d)", b, r.hs, r.ws, r.offset, r.flags);
        const long long bytes = (long long)F * r.hs * r.ws * 3;
        SSM_REQUIRE(r.offset <= frames_bytes && bytes <= frames_bytes - r.offset,
                    "clip_batch_from_u8: sample %d: %d frames of %dx%d at offset %lld leave the buffer of %lld bytes", b, F, r.hs, r.ws, r.offset,
                    frames_bytes);
        const int h = (r.flags & SSM_CLIP_TRANSPOSE) ? r.ws : r.hs, w = (r.flags & SSM_CLIP_TRANSPOSE) ? r.hs : r.ws;
        SSM_REQUIRE(r.y1 >= 0 && r.x1 >= 0 && r.y1 <= h - th && r.x1 <= w - tw,
                    "clip_batch_from_u8: sample %d: the %dx%d crop at (%d,%d) leaves the %dx%d frame", b, th, tw, r.y1, r.x1, h, w);
    }
    const int vec_in = (reinterpret_cast<size_t>(frames) % 4 == 0 && frames_bytes % 4 == 0) ? 1 : 0;
    const int vec_out = (tw % 4 == 0 && ssm::aligned16(input) && ssm::aligned16(target)) ? 1 : 0;
    Norm3 nm;
    for (int c = 0; c < 3; ++c) nm.m[c] = mean3[c], nm.s[c] = std3[c];
    const dim3 grid((unsigned)(((long long)th * ((tw + 3) / 4) + 255) / 256), B * F);
    SSM_LAUNCH(clip_batch_from_u8_kernel, grid, dim3(256), 0, (hipStream_t)stream, frames, table_dev, input, target, F, n_in, th, tw, nm, vec_in,
               vec_out);
    return ssm::check_launch("ssm_clip_batch_from_u8_fwd");
}
