/* ssm_hip.h - C ABI of libssm_hip.so: the MI355X (gfx950) replacement for the
 * stock-PyTorch operators on the Super SloMo frame-pair -> intermediate-frame
 * path.  Plain pointers and sizes only; no torch types.  Every entry point
 * cites the reference interface it replaces (paths relative to the reference
 * repository root).
 *
 * Conventions
 *  - all tensors are fp32 device memory owned by the caller; the library never
 *    allocates or frees device memory and keeps no pointer past return - with
 *    ONE exception the caller opts into: a launch program (ssm_program_*)
 *    keeps a copy of the argument values, pointers included, of every launch
 *    it recorded until ssm_program_destroy; the buffers they point to must
 *    outlive the program's last ssm_program_run;
 *  - every call is asynchronous on `stream` (a hipStream_t passed as void*) and
 *    re-entrant.  It launches on the CALLING THREAD's current device
 *    (hipGetDevice), which must own `stream` and every pointer passed; the
 *    library never calls hipSetDevice and keeps no "current device" of its
 *    own.  One process may drive several GPUs from several host threads (the
 *    reference's torch.nn.DataParallel replica threads, scripts/main.py:74-76:
 *    each thread has set its device): per-device state - the opt-in of a
 *    kernel to more than 64 KiB of dynamic LDS - is keyed on (kernel, device)
 *    and taken on a thread's first launch there (csrc/ssm_common.h
 *    reserve_lds; tests/test_build_fences_cpu.py fences process-wide guards);
 *  - return value 0 = ok, negative = SSM_E_* ; ssm_last_error_string() holds a
 *    message for the calling thread.  Nothing throws or exits.  The Python side
 *    turns non-zero codes into RuntimeError, mirroring the reference's
 *    assert/exception convention (scripts/utils/validators.py).
 *
 * Tensor views
 *  A `ssm_view` addresses logical element (b,c,y,x) at
 *      ptr[b*sb + c*sc + y*sh + x]           (strides in floats, x-stride 1)
 *  so the same entry points take plain contiguous NCHW (sh=W, sc=H*W,
 *  sb=C*H*W), channel slices of it, batch-broadcast tensors (sb=0) and the
 *  library's "padded plane" layout.
 *
 * Padded-plane layout (what the convolutions read)
 *  [B][C][Hp][Wp] with Hp = H + 2*SSM_PADY, Wp = roundup4(W + 2*SSM_PADX),
 *  the image at rows SSM_PADY.., cols SSM_PADX.. and an all-zero frame around
 *  it.  `ptr` of such a view points at the first INTERIOR element, is 16-byte
 *  aligned, and sh/sc/sb are multiples of 4.  The zero frame implements the
 *  convolution's zero padding (scripts/models/layers.py:22-31) with no bounds
 *  test in the kernel.  Kernels only ever write interiors, so a buffer zeroed
 *  once stays valid.  The DIRECT-form kernels (ssm_conv2d_*, ssm_conv2d_hl8_*)
 *  read a tile's overshoot past the map unpredicated: their inputs must be
 *  readable for SSM_TAIL_SLACK_FLOATS past the last element; what is read
 *  there only feeds outputs that are not stored.  The weight-gradient kernels
 *  (ssm_conv2d_wgrad*, every output of which sums over the whole map) read
 *  dZ inside the image only and the activations inside their plane rows only
 *  (rows -p .. H + p - 1 with p = (k - 1) / 2, columns -4 .. roundup4(W +
 *  SSM_PADX) - 1: the zero frame and the row's round-up padding): a staging
 *  step that reaches further - the last pixel group of a ragged row, which
 *  would meet nothing but zeroed dZ, and 0 * NaN is NaN - stages zeros, so
 *  nothing behind the last plane can reach a sum
 *  (tests/test_hip_wgrad_exact.py poisons it).  The Winograd-form kernels
 *  (ssm_wino_*, ssm_wino1d_*, ssm_wino4_*, ssm_wino5_*, ssm_wino7_*) never read
 *  outside the padded plane: a tile's transform mixes its whole input patch
 *  into every output, so overshoot rows / 16-byte pieces are fetched from the
 *  zero frame instead (tests/test_hip_overshoot.py poisons the memory behind
 *  the last plane with NaN).
 */
#ifndef SSM_HIP_H
#define SSM_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SSM_PADX 4
#define SSM_PADY 3
#define SSM_TAIL_SLACK_FLOATS (1 << 16)

#define SSM_OK 0
#define SSM_E_ARG (-1)      /* bad shape / alignment / unsupported size      */
#define SSM_E_LAUNCH (-2)   /* HIP reported a launch error                   */
#define SSM_E_UNSUPPORTED (-3)

#define SSM_FLAG_LRELU 1    /* apply LeakyReLU(slope) after bias             */
#define SSM_FLAG_FP16_FAST 2 /* HL8 conv: hi*hi product only (plain fp16 inputs) */
#define SSM_FLAG_Q8 4        /* HL8 conv on Q8 operands: 1 fp16 MFMA + 2 block-scaled fp8 MFMAs per product */
#define SSM_FLAG_MASK 8      /* the `add` view of an *_add_fwd entry point (ssm_wino_conv2d_add_fwd, ssm_wino4_conv2d_add_fwd, ssm_wino5_conv2d_add_fwd,
                              * ssm_splitk_finish_fwd) is a MASK source m instead of a pre-activation addend: out = conv(x) * (m > 0 ? 1 :
                              * slope), no activation (SSM_FLAG_LRELU must be clear).  The training step's data gradients use it: the
                              * gradient wrt a layer's input leaves the convolution as dZ of the layer that produced that input -
                              * dX * LeakyReLU'(its output) - and the separate ssm_lrelu_bwd pass over it disappears (autograd of
                              * layers.conv's LeakyReLU(0.1), scripts/models/layers.py:21-33)                                              */

typedef struct ssm_view {
    float *ptr;
    long long sb, sc;   /* batch / channel stride, floats */
    int sh;             /* row stride, floats             */
} ssm_view;

/* "HL8" activation: every fp32 value x is carried as hi = fp16(x), lo = fp16(x - hi).
 * [B][C/8][2 = hi|lo][Hp][Wp][8 x fp16]; a pixel's 8 channels of one part are one 16-byte
 * unit (= one fp16 MFMA operand fragment).  Same zero frame / slack rules as the fp32 padded
 * planes.  Strides in 16-byte pixels; ptr = first INTERIOR pixel of group 0, hi part.      */
typedef struct ssm_hview {
    void *ptr;
    long long sb, sg, sp;   /* batch stride, channel-group stride, hi->lo stride */
    int sh;                 /* row stride */
} ssm_hview;

int ssm_abi_version(void);
const char *ssm_last_error_string(void);

/* Padded-plane geometry for an HxW image. */
void ssm_plane_dims(int H, int W, int *Hp, int *Wp);

/* Strided copy of a [B,C,H,W] block between two views (NCHW <-> padded plane,
 * channel slices, torch.cat by writing at a channel offset).                */
int ssm_copy_view(ssm_view src, ssm_view dst, int B, int C, int H, int W, void *stream);

/* Which tile configuration ssm_conv2d_fwd will use for this problem (kernel size,
 * output channels, batch, map size, fused pool or not):
 * BN = output-channel block the weights must be packed for, CK = input-channel
 * chunk (Cin and the first cat source must be multiples of it).             */
int ssm_conv_config(int k, int Cout, int B, int H, int W, int pool, int *BN, int *CK);
/* The same with the input channel count and the fused-upsample form taken into account (what ssm_conv2d_fwd /
 * ssm_conv2d_ups_fwd evaluate at launch: an estimate of the launch duration per tile configuration from the
 * workgroup count against the 512 resident slots of the chip, the MFMAs per workgroup and the tile overshoot).
 * kind = index of the configuration (diagnostics).  Pack filters for the BN / CK returned HERE.               */
int ssm_conv_plan(int k, int Cin, int Cout, int B, int H, int W, int pool, int ups, int *kind, int *BN, int *CK);
/* Tests / tuning only: force tile configuration `kind` for its kernel size (-1 = automatic).  Process-wide.
 * Returns the number of configurations.                                                                     */
int ssm_conv_force_kind(int kind);

/* Number of floats of the packed filter / packed bias for that configuration. */
size_t ssm_packed_weight_floats(int Cout, int Cin_padded, int k, int BN);
size_t ssm_packed_bias_floats(int Cout, int BN);

/* OIHW fp32 filter (the reference's state-dict layout) ->
 * [Cout/BN][Cin_padded][k*k][BN], zero-filled where padded.  Device to device. */
int ssm_pack_weights(const float *w_oihw, const float *bias, float *w_packed, float *bias_packed,
                     int Cout, int Cin, int Cin_padded, int k, int BN, void *stream);

/* Replaces layers.conv = Conv2d(stride 1, pad (k-1)/2, bias) [+ LeakyReLU(0.1)]
 * (scripts/models/layers.py:21-33) and the bare final_conv
 * (scripts/models/flow_computation.py:145-153).  fp32 implicit GEMM on
 * v_mfma_f32_32x32x2_f32.  k in {3,5,7}.
 *   x1,C1 / x2,C2 : input = torch.cat([x1, x2], dim=1) without materialising it
 *                   (fuse_conv, flow_computation.py:271-272); C2 may be 0.
 *                   Both padded-plane views with identical sh/sc.
 *   y             : any view, [B,Cout,H,W]
 *   pool          : optional (ptr NULL = off) view [B,Cout,H/2,W/2] that
 *                   receives avg_pool2(y) (scripts/models/layers.py:60-63)
 *                   fused into the epilogue.                                */
int ssm_conv2d_fwd(ssm_view x1, int C1, ssm_view x2, int C2, const float *w_packed,
                   const float *bias_packed, ssm_view y, ssm_view pool, int B, int H, int W,
                   int Cout, int k, float slope, int flags, void *stream);

/* Fused  conv3x3( F.upsample(torch.cat([a, b], 1), size=(2h,2w), mode="bilinear") )  - the decoder step of
 * scripts/models/flow_computation.py:244-247 (lambdas :92-137; flow_interpolation.py:92-141,224-231) - in exact
 * fp32 (v_mfma_f32_32x32x2_f32).  a [B,C1,H/2,W/2], b [B,C2,H/2,W/2] LOW-res padded-plane views (C2 may be 0, b may
 * be batch-broadcast), H, W = OUTPUT size (even).  The concatenated, upsampled tensor is never materialised: each
 * workgroup expands the low-res chunk it staged into the hi-res patch in LDS (align_corners=False half-pixel rule,
 * edge-clamped sources, zeros outside the image = the convolution's padding).  Filters: ssm_pack_weights for the
 * BN / CK of ssm_conv_plan(3, C1+C2, Cout, B, H, W, 0, 1, ...).                                                  */
int ssm_conv2d_ups_fwd(ssm_view a, int C1, ssm_view b, int C2, const float *w_packed, const float *bias_packed,
                       ssm_view y, int B, int H, int W, int Cout, float slope, int flags, void *stream);

/* The two convolutions above with a pre-activation addend: y = act(conv(x) + bias + add[b / add_div]), add = a view
 * [B / add_div, Cout, H, W].  For the parts of a convolution's input that do not depend on the batch index - the reference
 * evaluates stage 2 once per interpolation time t (evaluate_interpolation_results.py:234-242), but the image channels of its
 * first convolution's 16-channel input (flow_interpolation.py:364-367: channels 0:3 and 13:16) and the stage-1 half of the
 * cross-skip concat in front of conv7a (flow_interpolation.py:98-101,224-231) are the same for every t of a pair: their
 * partial sums are computed once per pair by a plain call and enter the per-t launches here.  add.ptr NULL = the plain form.
 * The direct kernels read the addend unpredicated: Cout must be a multiple of the plan's BN and add a padded-plane view
 * (readable frame / tail slack for the tile overshoot); the Winograd kernels predicate their reads.                       */
int ssm_conv2d_add_fwd(ssm_view x1, int C1, ssm_view x2, int C2, const float *w_packed, const float *bias_packed, ssm_view y,
                       ssm_view pool, ssm_view add, int add_div, int B, int H, int W, int Cout, int k, float slope, int flags,
                       void *stream);
int ssm_conv2d_ups_add_fwd(ssm_view a, int C1, ssm_view b, int C2, const float *w_packed, const float *bias_packed, ssm_view y,
                           ssm_view add, int add_div, int B, int H, int W, int Cout, float slope, int flags, void *stream);

/* ---- the same 3x3 convolution as Winograd F(2x2,3x3), all arithmetic fp32 (v_mfma_f32_32x32x2_f32) ---------------
 * Same operator and operand layout as ssm_conv2d_fwd / ssm_conv2d_ups_fwd for k = 3 (layers.conv,
 * scripts/models/layers.py:21-33; decoder step scripts/models/flow_computation.py:244-247), evaluated as
 * Y = A^T [ sum_cin (G g G^T) .* (B^T d B) ] A per 2x2 output tile: 16 instead of 36 multiplies per (cin, cout, 4 outputs),
 * i.e. 2.25x fewer matrix-core cycles; in fp32 the result differs from the direct form by rounding only (about as much as
 * a different summation order; profiles/DESIGN_history_r1-r3.md 3.2d).  Any H, W (r6: odd widths too - the last tile of a row stores its lone column by itself, the zero frame stays
 * untouched; the fused pool and the fused upsample need even sizes); Cin and the first cat source multiples of CK.
 * ssm_wino_plan: tile configuration for the problem (ups: the fused-upsample entry point; BN = cout block to pack for, CK =
 * channel chunk); two kernel forms - one workgroup per CU with 16 frequency accumulators per wave, or two per CU with 8.
 * ssm_wino_pack_weights: OIHW fp32 3x3 filter -> U = G g G^T as [Cout/BN][Cin][4][BN][4] (+ bias padded to BN).          */
int ssm_wino_plan(int Cin, int Cout, int B, int H, int W, int ups, int *kind, int *BN, int *CK);
int ssm_wino_force_kind(int kind);       /* tests / tuning only (-1 = automatic); returns the number of configurations */
size_t ssm_wino_packed_weight_floats(int Cout, int Cin, int BN);
int ssm_wino_pack_weights(const float *w_oihw, const float *bias, float *w_packed, float *bias_packed, int Cout, int Cin,
                          int BN, void *stream);
int ssm_wino_conv2d_fwd(ssm_view x1, int C1, ssm_view x2, int C2, const float *w_packed, const float *bias_packed,
                        ssm_view y, ssm_view pool, int B, int H, int W, int Cout, float slope, int flags, void *stream);
int ssm_wino_conv2d_ups_fwd(ssm_view a, int C1, ssm_view b, int C2, const float *w_packed, const float *bias_packed,
                            ssm_view y, int B, int H, int W, int Cout, float slope, int flags, void *stream);

/* Split-K form of the two convolutions above for launches that leave most of the chip idle (config 3's bottleneck layers: 512 -> 512
 * channels on 22x22 / 11x11 maps at batch 2 are 96-192 workgroups, each walking every input channel).  ssm_wino_splitk_plan proposes
 * KS in {1, 2, 4, 8} (1: do not split; $SSM_WINO_SPLITK=0: always 1) for a filter packed with BN couts per block;
 * ssm_wino_conv2d_splitk_fwd (ups = 1: conv3x3(upsample2x(cat[a, b])), H x W the output) runs KS workgroups per output tile, workgroup
 * ks summing input channels [ks, ks + 1) * Cin / KS, and stores the raw sums (the bias with ks = 0, no activation) as batch entry
 * ks * B + b of `part` ([KS * B, Cout, H, W] padded planes owned by the caller); ssm_splitk_finish_fwd (csrc/ssm_elem.hip) adds the KS
 * partial maps in the order ks = 0, 1, ... (deterministic), then the optional addend [B / add_div, C, H, W], LeakyReLU (flags) and the
 * optional fused 2x2 mean - layers.conv / avg_pool of scripts/models/layers.py:21-33,60-63 as before, in two launches.              */
int ssm_wino_splitk_plan(int Cin, int Cout, int B, int H, int W, int ups, int BN, int *KS);
int ssm_wino_conv2d_splitk_fwd(ssm_view x1, int C1, ssm_view x2, int C2, const float *w_packed, const float *bias_packed, ssm_view part,
                               int KS, int ups, int B, int H, int W, int Cout, int BN, void *stream);
int ssm_splitk_finish_fwd(ssm_view part, int KS, ssm_view y, ssm_view pool, ssm_view add, int add_div, int B, int C, int H, int W,
                          float slope, int flags, void *stream);
/* The direct-form twin (csrc/ssm_conv.hip) for the maps no Winograd form takes (odd widths: config 3's 11x11 bottleneck): the same
 * convolution as ssm_conv2d_fwd - ONE source when KS > 1 (C2 must be 0: the kernel offsets its first source by the split's channel
 * range; two sources are accepted with KS = 1 only), no fused pool - with KS workgroups per output tile; `part` and the finishing
 * launch as above (ssm_splitk_finish_fwd takes odd widths too).  ssm_conv_splitk_plan: KS for the tile configuration the filter was
 * packed for (1: do not split; $SSM_CONV_SPLITK=0: always 1).                                                                    */
int ssm_conv_splitk_plan(int k, int Cin, int Cout, int B, int H, int W, int *KS);
/* Run-time twin of $SSM_WINO_SPLITK / $SSM_CONV_SPLITK for the two plan functions: 1 = on, 0 = off, -1 = leave.  Returns the previous
 * state as (wino | conv << 1).  A split reorders a layer's fp32 sum over the input channels: tests A/B it in one process.            */
int ssm_splitk_enable(int wino, int conv);
int ssm_conv2d_splitk_fwd(ssm_view x1, int C1, ssm_view x2, int C2, const float *w_packed, const float *bias_packed, ssm_view part,
                          int KS, int B, int H, int W, int Cout, int k, void *stream);
/* ... with the pre-activation addend of ssm_conv2d_add_fwd (8-byte aligned view). */
int ssm_wino_conv2d_add_fwd(ssm_view x1, int C1, ssm_view x2, int C2, const float *w_packed, const float *bias_packed, ssm_view y,
                            ssm_view pool, ssm_view add, int add_div, int B, int H, int W, int Cout, float slope, int flags,
                            void *stream);
int ssm_wino_conv2d_ups_add_fwd(ssm_view a, int C1, ssm_view b, int C2, const float *w_packed, const float *bias_packed, ssm_view y,
                                ssm_view add, int add_div, int B, int H, int W, int Cout, float slope, int flags, void *stream);

/* ---- the 3x3 convolution as Winograd F(4x4,3x3), all arithmetic fp32 (v_mfma_f32_16x16x4_f32) ------------------------------
 * Same operator and operand layout as ssm_wino_conv2d_add_fwd / ssm_wino_conv2d_ups_add_fwd (layers.conv, scripts/models/layers.py:21-33;
 * decoder step scripts/models/flow_computation.py:244-247), evaluated per 4x4 output tile from its 6x6 input patch over the points
 * {0, +-1, +-2, inf}: 36 instead of 144 multiplies per (cin, cout, 16 outputs) - 1.78x fewer matrix-core cycles than F(2x2,3x3); in
 * fp32 a single layer sits ~1e-5 from a float64 evaluation at unit output scale (per-layer bar 5e-5), the pair -> frame path at
 * 736x1280 is unchanged within its fp32 noise (tests/emulate_winograd_f44_precision.py; profiles/DESIGN_history_r1-r3.md 3.2f).
 * Cin and the first cat source multiples of 4, Cout a multiple of 32; any H, W (fused upsample: even).
 * ssm_wino4_pack_weights: OIHW fp32 3x3 filter -> U = G g G^T as [Cout/32][Cin][9][32][4] (+ bias).
 * Inputs must be padded planes; nothing outside them is read (tile overshoot is fetched from the zero frame), any row stride.          */
int ssm_wino4_plan(int Cin, int Cout, int B, int H, int W, int ups, int *kind, int *BN, int *CK);
int ssm_wino4_preferred(int Cin, int Cout, int B, int H, int W, int ups);   /* 1: modelled faster than F(2x2,3x3) for this problem */
double ssm_wino_estimate(int Cin, int Cout, int B, int H, int W, int ups);     /* modelled cycles of ssm_wino_conv2d_*_fwd (-1: unsupported) */
int ssm_wino4_force_kind(int kind);      /* tests / tuning only (-1 = automatic); returns the number of configurations */
size_t ssm_wino4_packed_weight_floats(int Cout, int Cin);
int ssm_wino4_pack_weights(const float *w_oihw, const float *bias, float *w_packed, float *bias_packed, int Cout, int Cin, void *stream);
int ssm_wino4_conv2d_add_fwd(ssm_view x1, int C1, ssm_view x2, int C2, const float *w_packed, const float *bias_packed, ssm_view y,
                             ssm_view pool, ssm_view add, int add_div, int B, int H, int W, int Cout, float slope, int flags,
                             void *stream);
int ssm_wino4_conv2d_ups_add_fwd(ssm_view a, int C1, ssm_view b, int C2, const float *w_packed, const float *bias_packed, ssm_view y,
                                 ssm_view add, int add_div, int B, int H, int W, int Cout, float slope, int flags, void *stream);
/* conv3x3(upsample2x(cat[a, b])) (scripts/models/flow_computation.py:244-247; layers.conv, scripts/models/layers.py:21-33) in its SUB-PIXEL form
 * away from the map's border (r5).  The operator is linear in the low-res input: output parity (pa, pb) of real channel c is a plain 3x3
 * convolution of the LOW-res map with the effective filter M_pa W_c M_pb^T (bilinear weights 1/4, 3/4 folded into the taps), so the layer is
 *   ssm_wino4_conv2d_shuffle_fwd: a 3x3 convolution with 4 Cout effective output channels, channel 4 c + 2 pa + pb, whose 4x4 low-res tiles are
 *     stored as 8x8 blocks of the 2H x 2W output (pixel-shuffle store).  x1 / x2: low-res padded-plane views AT THE REGION'S ORIGIN (the region's
 *     neighbours must be the real neighbouring pixels: it is the map's interior), y: the full-resolution output view at twice that origin,
 *     H x W: the low-res region, w_packed / bias_packed: ssm_wino4_pack_weights of the effective filter (bias repeated per parity).
 * where the bilinear rule does not clamp and the convolution does not zero-pad, i.e. everywhere but on the border ring, which
 *   ssm_wino4_conv2d_ups_border_fwd: the fused-upsample kernel (arguments of ssm_wino4_conv2d_ups_add_fwd) restricted to the workgroup tiles
 *     of SSM_WINO4_BORDER_TH x SSM_WINO4_BORDER_TW output pixels on the map's border ring
 * computes.  Together they equal ssm_wino4_conv2d_ups_add_fwd (no addend) when the shuffle launch covers exactly the interior tiles. */
#define SSM_WINO4_BORDER_TH 16
#define SSM_WINO4_BORDER_TW 32
int ssm_wino4_conv2d_shuffle_fwd(ssm_view x1, int C1, ssm_view x2, int C2, const float *w_packed, const float *bias_packed, ssm_view y, int B,
                                 int H, int W, int Cout4, float slope, int flags, void *stream);
int ssm_wino4_conv2d_ups_border_fwd(ssm_view a, int C1, ssm_view b, int C2, const float *w_packed, const float *bias_packed, ssm_view y, int B,
                                    int H, int W, int Cout, float slope, int flags, void *stream);

/* ---- conv3x3(upsample2x(cat[a, b])) as a 1x1 GEMM at low resolution, taps after the upsample (v_mfma_f32_32x32x2_f32) ---------
 * The decoder step of scripts/models/flow_computation.py:244-247 (layers.conv, scripts/models/layers.py:21-33).  Bilinear upsampling acts
 * per channel, a filter tap's channel mixing is a matrix, and the two commute:
 *   conv3x3(up(x))(Y, X) = bias + sum_{u,v} [ (Y+u-1, X+v-1) inside the map ] up(W[:, :, u, v] . x)(Y+u-1, X+v-1)
 * so the layer is one GEMM Cin -> 9 Cout over the LOW-res pixels (9/36 of the direct form's multiply-adds, no transforms) into a scratch set of
 * planes [B][9 Cout][H/2][.], and a memory-bound pass that gathers the nine shifted bilinear samples (ATen's half-pixel rule, edge-clamped;
 * zero where the tap lies outside the map), adds bias and the optional pre-activation addend [B / add_div] and applies LeakyReLU.  All
 * arithmetic fp32; a single layer sits ~2e-6 from a float64 evaluation at unit output scale.  Cout a multiple of 32, H and W (the OUTPUT
 * size) even, any Cin / C1 (whole 16-channel chunks take the fast loader).  a, b: LOW-res padded-plane views as for ssm_conv2d_ups_add_fwd
 * (b may be batch-broadcast, sb = 0); tile overshoot is read from the frame / the tail slack and never stored.  Only interiors of scratch
 * and y are written; no scratch element is read that the same call did not write.  `bias` is the layer's plain [Cout] bias.          */
int ssm_upgemm_supported(int Cin, int Cout, int H, int W, int k);      /* flow_computation.py:244-247: can the layer (H x W output) run in this form? */
int ssm_upgemm_preferred(int Cin, int Cout, int B, int h, int w);      /* flow_computation.py:244-247: 1 where GEMM + combine measured faster than F(4x4,3x3); h x w = the LOW-res map */
int ssm_upgemm_force_kind(int kind);      /* flow_computation.py:244-247: tests / tuning only, the GEMM's tile configuration (-1 = automatic); returns their number */
size_t ssm_upgemm_packed_weight_floats(int Cout, int Cin);      /* flow_computation.py:244-247 */
/* flow_computation.py:244-247: OIHW fp32 3x3 filter -> the GEMM's A operand [9 Cout / 128][Cin rounded up to 16][128], row = tap Cout + cout */
int ssm_upgemm_pack_weights(const float *w_oihw, float *w_packed, int Cout, int Cin, void *stream);
/* flow_computation.py:244-247: floats of the scratch planes [B][9 Cout][h][w rounded up to 4] of a launch with a h x w LOW-res map */
size_t ssm_upgemm_scratch_floats(int Cout, int B, int h, int w);
/* flow_computation.py:244-247: both launches on `stream`; scratch: view {ptr, sb >= 9 Cout sc, sc >= h sh, sh >= w, all multiples of 4} */
int ssm_upgemm_conv2d_ups_add_fwd(ssm_view a, int C1, ssm_view b, int C2, const float *w_packed, const float *bias, ssm_view scratch, ssm_view y,
                                  ssm_view add, int add_div, int B, int H, int W, int Cout, float slope, int flags, void *stream);

/* ---- the 7x7 / 5x5 convolutions as one-dimensional Winograd along x, all arithmetic fp32 (v_mfma_f32_32x32x2_f32) ----------
 * Same operator and operand layout as ssm_conv2d_add_fwd for k = 7 / 5 (layers.conv, scripts/models/layers.py:21-33; the layers
 * conv1a/conv1b (k = 7) and conv2a/conv2b (k = 5) of both U-Nets, scripts/models/flow_computation.py:36-45 and
 * flow_interpolation.py:36-45; fused 2x2 mean, layers.py:60-63), evaluated as F(2,7) / F(4,5) along x - eight frequencies over the
 * points {0, +-1, +-2, +-1/2, inf} - and in the direct form along y: 8 multiplies per 2 (k = 7) / 4 (k = 5) outputs and filter
 * row instead of 14 / 20, i.e. 1.75x / 2.5x fewer matrix-core cycles; in fp32 the result differs from the direct form by
 * rounding only (a single layer: 5-8e-6 at unit output scale, tests/emulate_winograd_1d_precision.py; profiles/DESIGN_history_r1-r3.md 3.2e).
 * One input source (these layers have no concat); Cin a multiple of CK (= 2; pad the view), Cout a multiple of BN.
 * ssm_wino1d_plan: tile configuration (BN = cout block to pack for, CK = channel chunk).
 * ssm_wino1d_pack_weights: OIHW fp32 filter -> U[ky] = G g[ky] as [Cout/BN][CinP][k][2][BN][4] (+ bias padded to BN).
 * Outputs, addend and pooled outputs move as aligned 8- / 16-byte pieces when the views allow (W a multiple of 2 / 4 and
 * aligned strides: padded planes always do), element by element otherwise.                                                    */
int ssm_wino1d_plan(int k, int Cin, int Cout, int B, int H, int W, int *kind, int *BN, int *CK);
int ssm_wino1d_force_kind(int kind);     /* tests / tuning only (-1 = automatic); returns the number of configurations */
size_t ssm_wino1d_packed_weight_floats(int Cout, int CinP, int k, int BN);
int ssm_wino1d_pack_weights(const float *w_oihw, const float *bias, float *w_packed, float *bias_packed, int Cout, int Cin,
                            int CinP, int k, int BN, void *stream);
int ssm_wino1d_conv2d_add_fwd(ssm_view x, int Cin, const float *w_packed, const float *bias_packed, ssm_view y, ssm_view pool,
                              ssm_view add, int add_div, int B, int H, int W, int Cout, int k, float slope, int flags, void *stream);

/* ---- the 7x7 convolutions as a blocked two-dimensional Winograd form, all arithmetic fp32 (v_mfma_f32_16x16x4_f32) ----------
 * Same operator and operand layout as ssm_wino1d_conv2d_add_fwd for k = 7 (layers.conv, scripts/models/layers.py:21-33; conv1a /
 * conv1b of both U-Nets, scripts/models/flow_computation.py:36-45 and flow_interpolation.py:36-45; fused 2x2 mean, layers.py:60-63;
 * pre-activation addend for the hoisted part of stage 2's conv1a).  The 7x7 filter (zero-padded to 8x8) is 2x2 blocks of 4x4 taps;
 * each block is a F(4x4,4x4) Winograd filter over the seven points {0, +-1, +-2, 1/2, inf}, and because the blocks of a 4x4 output tile
 * read input windows that are whole tiles apart, one input transform per window position serves all four: 4 x 49 multiplies per 16
 * outputs and (cin, cout) = 12.25 per output against 28 for F(2,7) and 49 for the direct form (csrc/ssm_wino7.hip).
 * In fp32 the result differs from the direct form by rounding only (a 32-channel layer: 2e-6 rms / 3e-5 max at unit output scale).
 * One input source, any Cin >= 1 (a k-step is the four blocks of one channel: no channel padding); Cout a multiple of 32.
 * Inputs are padded planes; nothing outside them is read (tile overshoot and the bottom window's row H + 3 come from the zero frame).
 * ssm_wino7_pack_weights: OIHW fp32 7x7 filter -> U_b = G g_b G^T as [ceil(Cout/32)][Cin][14 quads][4 blocks][32][4] (+ bias, whole
 * 32-channel blocks).  Cout may be any positive count there: the channels up to the next multiple of 32 are packed as zeros, and the
 * convolution is then launched with that padded count on an output view that holds them (the data gradient of stage 2's conv1a).     */
int ssm_wino7_plan(int Cin, int Cout, int B, int H, int W, int *kind);
int ssm_wino7_force_kind(int kind);      /* tests / tuning only (-1 = automatic); returns the number of configurations */
size_t ssm_wino7_packed_weight_floats(int Cout, int Cin);
int ssm_wino7_pack_weights(const float *w_oihw, const float *bias, float *w_packed, float *bias_packed, int Cout, int Cin, void *stream);
int ssm_wino7_conv2d_add_fwd(ssm_view x, int Cin, const float *w_packed, const float *bias_packed, ssm_view y, ssm_view pool,
                             ssm_view add, int add_div, int B, int H, int W, int Cout, float slope, int flags, void *stream);

/* ---- the 5x5 convolutions as two-dimensional Winograd F(4x4,5x5), all arithmetic fp32 (v_mfma_f32_16x16x4_f32) ------------------
 * Same operator and operand layout as ssm_wino1d_conv2d_add_fwd for k = 5 (layers.conv, scripts/models/layers.py:21-33; conv2a /
 * conv2b of both U-Nets, scripts/models/flow_computation.py:43-45; fused 2x2 mean, layers.py:60-63): the eight points
 * {0, +-1, +-2, +-1/2, inf} of the 1-D F(4,5) form on BOTH axes - 64 multiplies per 16 outputs and (cin, cout) = 4 per output
 * against 10 for F(4,5) along x and 25 for the direct form (csrc/ssm_wino5.hip).  In fp32 the result differs from the
 * direct form by rounding only (a 64-channel layer: 3e-6 rms / 3e-5 max at unit output scale).
 * One input source; Cin a multiple of 4 (pad the view; pack with CinP), Cout a multiple of 32.  Inputs are padded planes; nothing
 * outside them is read (tile overshoot comes from the zero frame).
 * ssm_wino5_pack_weights: OIHW fp32 5x5 filter -> U = G g G^T as [Cout/32][CinP/4][16 quads][4 channels][32][4] (+ bias).          */
int ssm_wino5_plan(int Cin, int Cout, int B, int H, int W, int *kind);
int ssm_wino5_force_kind(int kind);      /* tests / tuning only (-1 = automatic); returns the number of configurations */
size_t ssm_wino5_packed_weight_floats(int Cout, int CinP);
int ssm_wino5_pack_weights(const float *w_oihw, const float *bias, float *w_packed, float *bias_packed, int Cout, int Cin, int CinP,
                           void *stream);
int ssm_wino5_conv2d_add_fwd(ssm_view x, int Cin, const float *w_packed, const float *bias_packed, ssm_view y, ssm_view pool,
                             ssm_view add, int add_div, int B, int H, int W, int Cout, float slope, int flags, void *stream);

/* ---- every fp32 filter of a U-Net repacked by one launch (training: the parameters change each optimizer step) ------------
 * A job = one convolution's OIHW parameter -> its packed form (algo: the per-layer pack entry point it replaces, same arithmetic,
 * same layout).  transposed: pack the DATA-GRADIENT filter of the forward parameter, W'[ci][co][ky][kx] = W[co][ci][k-1-ky][k-1-kx]
 * (the adjoint of layers.conv, scripts/models/layers.py:21-33, is the same convolution on it), read straight from the forward
 * tensor; Cout / Cin are then the data-gradient convolution's (Cout = the forward layer's input channels), bias NULL = zeros.
 * first = sum of max(total, nbias) over the preceding jobs.                                                                   */
enum { SSM_PACK_DIRECT = 0, SSM_PACK_WINO = 1, SSM_PACK_WINO1D = 2, SSM_PACK_WINO4 = 3, SSM_PACK_WINO7 = 4, SSM_PACK_WINO5 = 5 };
typedef struct {
    const float *w;      /* OIHW parameter */
    const float *bias;   /* or NULL */
    float *wp, *bp;      /* packed filter, packed bias */
    int Cout, Cin, CinP, k, BN, algo, transposed, nbias;
    long long first, total;
} ssm_pack32_job;
/* (a thread stores four packed elements: every job's `first` and `total` are multiples of 4 - BN is - and `wp` is 16-byte aligned) */
int ssm_pack32_weights_batch(const ssm_pack32_job *jobs_device, int n_jobs, long long total_elements, void *stream);
/* The F(2x2,3x3) jobs (algo 1) with k = 3, Cout % BN == 0, Cin % 16 == 0, BN <= 64 - most of a U-Net's bytes - by TILES of BN couts x 16
 * input channels: a workgroup reads its tile as contiguous rows and writes one contiguous run of the packed filter (the element-wise
 * kernel above fetches nine weights per thread from addresses Cin x 36 bytes apart).  Same job struct: `first` = the job's first tile,
 * `total` = its tiles = (Cout / BN) x (Cin / 16); max_bn = the largest BN of the table (LDS).  Bit-identical to the element-wise form. */
int ssm_pack32_wino_tiles_batch(const ssm_pack32_job *jobs_device, int n_jobs, long long total_tiles, int max_bn, void *stream);

/* ---- fp16-MFMA convolution on HL8 activations (v_mfma_f32_32x32x16_f16) ---------------
 * Same operator as ssm_conv2d_fwd.  Default mode evaluates a*b as a_hi*b_hi + a_hi*b_lo +
 * a_lo*b_hi with fp32 accumulation (fp32-grade products at 16/3 x the fp32-MFMA rate);
 * SSM_FLAG_FP16_FAST keeps only a_hi*b_hi (plain fp16 inputs; BASELINE config 5).
 * Filters are packed once with ssm_pack16_weights (scaled by a power of two `scale`;
 * pass wscale = 1/scale to the convolution).  Cin is padded to a multiple of 16.
 * Outputs: y_hl8 (ptr NULL = off) and/or y_f32 (ptr NULL = off), optional fused 2x2 mean
 * pool_hl8.
 * tests/test_hip_conv16_kinds.py runs every tile configuration in every operand mode on exact-integer and random data;
 * tests/test_hip_hl8_layout.py holds the layout, gather and HL8 element-wise kernels to float64 references.               */
int ssm_conv16_config(int k, int Cout, int W, int *BN, int *KYS);
/* Which tile configuration ssm_conv2d_hl8_fwd (ups = 0) / ssm_conv2d_ups_hl8_fwd (ups = 1; k = 3, W = output width) launches for
 * Cin = C1 + C2 input channels, with the packing dimensions the matching *_config call reports (flags: SSM_FLAG_Q8 selects the Q8
 * ones).  kind (diagnostics, tests): ups = 0: 0 H7, 1 H5, 2 H3N32, 3 H3N32D, 4 H3N64, 5 H3N128, 6 H3N128S, 7 H3N32V, 8 H3N32W;
 * ups = 1: 0 U3N32, 1 U3N64, 2 U3N128, 3 U3N128S.  Reads nothing but its arguments.                                            */
int ssm_conv16_plan(int k, int Cin, int Cout, int W, int ups, int flags, int *kind, int *BN, int *KYS);
size_t ssm_packed16_weight_halves(int Cout, int Cin_padded, int k, int BN);
int ssm_pack16_weights(const float *w_oihw, const float *bias, void *w_packed, float *bias_packed, int Cout,
                       int Cin, int Cin_padded, int k, int BN, int KYS, float scale, void *stream);
int ssm_conv2d_hl8_fwd(ssm_hview x1, int C1, ssm_hview x2, int C2, const void *w_packed,
                       const float *bias_packed, float wscale, ssm_hview y_hl8, ssm_view y_f32,
                       ssm_hview pool_hl8, int B, int H, int W, int Cout, int k, float slope, int flags,
                       void *stream);
/* Fused  conv3x3( F.upsample(torch.cat([a, b], 1), size=(2h,2w), mode="bilinear") )  - the decoder step of
 * scripts/models/flow_computation.py:244-247 (and :103-137) - on LOW-res HL8 inputs a [B,C1,H/2,W/2] and
 * b [B,C2,H/2,W/2] (C2 may be 0; b may be batch-broadcast).  H, W = OUTPUT size.  The concatenated, upsampled
 * tensor is never materialised: expander waves rebuild it tile by tile in LDS under the matrix waves' MFMAs.
 * Filters: the ssm_pack16_weights packing for (k=3, Cout) (independent of KYS).                              */
int ssm_conv16_ups_config(int Cout, int W, int *BN, int *KYS);
int ssm_conv2d_ups_hl8_fwd(ssm_hview a, int C1, ssm_hview b, int C2, const void *w_packed,
                           const float *bias_packed, float wscale, ssm_hview y_hl8, ssm_view y_f32, int B, int H,
                           int W, int Cout, float slope, int flags, void *stream);
/* Q8 operand form (SSM_FLAG_Q8 on the two convolution entry points): plane 1 of every pixel group holds
 * [8 x fp8 e4m3 (x) | 8 x fp8 ((x - fp16(x)) * 2^11)] instead of 8 x fp16(lo); a product is a_hi*b_hi on the fp16 matrix path
 * plus fp8(a)*fp8(b_lo) + fp8(a_lo)*fp8(b) on the block-scaled fp8 path (v_mfma_scale_f32_32x32x64_f8f6f4, K = 4 taps x 16
 * channels, E8M0 scale 2^-11 on the lo operand) - 1 + 2*(1/4) fp16-MFMA units per product instead of 3.  Same geometry,
 * strides and entry points as HL8; filters are packed by ssm_pack16q_weights for the tile ssm_conv16q_config reports.      */
int ssm_conv16q_config(int k, int Cout, int W, int *BN, int *KYS);
int ssm_conv16q_ups_config(int Cout, int W, int *BN, int *KYS);      /* tile of ssm_conv2d_ups_hl8_fwd with SSM_FLAG_Q8 */
size_t ssm_packed16q_weight_bytes(int Cout, int Cin_padded, int k, int BN, int KYS);
int ssm_pack16q_weights(const float *w_oihw, const float *bias, void *w_packed, float *bias_packed, int Cout, int Cin,
                        int Cin_padded, int k, int BN, int KYS, float scale, void *stream);
int ssm_flowinterp_inputs_hq8_fwd(ssm_view img6, ssm_view flow4, const float *t, ssm_hview out16, ssm_view flows4, int B, int H,
                                  int W, void *stream);      /* ssm_flowinterp_inputs_hl8_fwd with a Q8 output */
/* Sub-pixel form of the decoder's `F.upsample(cat([x, skip]), scale 2, bilinear)` + 3x3 conv (scripts/models/flow_computation.py:
 * 215-289, flow_interpolation.py:220-281): conv3x3(upsample2x(X)) is a plain 3x3 convolution of the LOW-res tensors with 4*Cr
 * outputs - one effective filter M_a * W * M_b^T per output parity (a, b), packed by the caller as channel (2a + b)*Cr + c - and a
 * pixel-shuffle store: channel (2a + b)*Cr + c of low-res pixel (y, x) lands at pixel (2y + a, 2x + b) of channel c of y_hl8
 * (transposed: (2x + b, 2y + a)).  y_hl8 points at the destination pixel of this launch's low-res pixel (0, 0); H, W = low-res
 * extent of the launch.  The rows / columns 0 and last need their own effective filters (bilinear clamping vs the convolution's
 * zero padding): the caller overwrites them from strip launches (H = 1 views; columns through ssm_hl8_gather_cols copies).
 * Q8 operands only (flags must carry SSM_FLAG_Q8).                                                                          */
int ssm_conv2d_hl8_subpixel_fwd(ssm_hview x1, int C1, ssm_hview x2, int C2, const void *w_packed, const float *bias_packed,
                                float inv_wscale, ssm_hview y_hl8, int B, int H, int W, int Cr, int transposed, float slope, int flags,
                                void *stream);
/* The main problem, the four border strips and the four corners of a sub-pixel decoder level as ONE launch: every problem is one
 * ssm_conv2d_hl8_subpixel_fwd call (all with the filter packing of ssm_conv16q_config(3, 4*Cr, wcfg)); skip_y / skip_x make a
 * problem leave the first and last row / column of its extent to the problem that owns them, so the outputs are disjoint and the
 * problems need no ordering.  ssm_conv16_subpixel_plan fills `table_host` (ssm_conv16_subpixel_table_bytes(n) bytes; copy it to
 * device memory once - it holds the raw pointers of the views) and block_start[n+1]; ssm_conv16_subpixel_run launches it.     */
typedef struct ssm_subpixel_problem {
    ssm_hview x1;
    int C1;
    ssm_hview x2;
    int C2;
    const void *w_packed;
    const float *bias_packed;
    float inv_wscale;
    ssm_hview y_hl8;
    int H, W;
    int transposed;
    int skip_y, skip_x;
} ssm_subpixel_problem;
size_t ssm_conv16_subpixel_table_bytes(int n);
int ssm_conv16_subpixel_plan(const ssm_subpixel_problem *problems, int n, int B, int Cr, int wcfg, float slope, int flags,
                             void *table_host, size_t table_bytes, int *block_start);
int ssm_conv16_subpixel_run(const void *table_device, int n, const int *block_start, int Cr, int wcfg, int Cin, void *stream);
/* Image columns of the Ga + Gb groups of a two-source HL8 / Q8 tensor as the rows of a zero-framed tensor (record copies, both
 * planes): dst rows 0..ncols-1 = columns col0.., and if col1 >= 0 dst rows ncols+1..2*ncols = columns col1.. (row ncols is left
 * alone: the zero gap between the two column strips' neighbourhoods).                                                          */
int ssm_hl8_gather_cols(ssm_hview a, int Ga, ssm_hview b, int Gb, ssm_hview dst, int B, int H, int col0, int ncols, int col1,
                        void *stream);
/* All filters of a U-Net packed (Q8 form) by ONE launch: the training step repacks every filter after each optimizer step
 * (scripts/main.py:188-197 updates the nn.Conv2d weights of scripts/models/layers.py:21-33 in place).  A job describes one
 * ssm_pack16q_weights call; transposed = 1 packs the data-gradient filter W'[co][ci][ky][kx] = w[ci][co][k-1-ky][k-1-kx] straight
 * from the forward OIHW tensor `w` (Cout/Cin are those of W'), bias = NULL packs zeros.  block_start = running sum of
 * row_blocks + bias_blocks (ssm_pack16q_job_blocks) over the preceding jobs; the job array lives in device memory.        */
typedef struct ssm_pack16q_job {
    const float *w;
    const float *bias;
    void *wp;
    float *bp;
    int Cout, Cin, CinP, k, BN, KYS;
    float scale;
    int transposed;
    int block_start, row_blocks;
} ssm_pack16q_job;
int ssm_pack16q_job_blocks(int Cout, int CinP, int k, int BN, int *row_blocks, int *bias_blocks);
int ssm_pack16q_weights_batch(const ssm_pack16q_job *jobs_device, int n_jobs, int total_blocks, void *stream);
int ssm_hq8_from_f32(ssm_view src, ssm_hview dst, int B, int C, int G, int H, int W, void *stream);
int ssm_hq8_to_f32(ssm_hview src, ssm_view dst, int B, int C, int G, int H, int W, void *stream);
/* fp32 view [B,C,H,W] <-> HL8 with G >= ceil(C/8) channel groups (extra channels are zeros). */
int ssm_hl8_from_f32(ssm_view src, ssm_hview dst, int B, int C, int G, int H, int W, void *stream);
int ssm_hl8_to_f32(ssm_hview src, ssm_view dst, int B, int C, int G, int H, int W, void *stream);

/* HL8 forms of the concat+bilinear-x2 and of compute_inputs (same semantics as the fp32 entry
 * points below; Ga/Gb = channel groups of 8).  ssm_flowinterp_inputs_hl8_fwd also writes the four
 * approximated flow channels (Ft1^ u,v | Ft0^ u,v) as fp32 `flows4` for ssm_synthesize_fwd.    */
int ssm_upsample2x_cat_hl8_fwd(ssm_hview a, int Ga, ssm_hview b, int Gb, ssm_hview y, int B, int h, int w,
                               void *stream);
int ssm_flowinterp_inputs_hl8_fwd(ssm_view img6, ssm_view flow4, const float *t, ssm_hview out16,
                                  ssm_view flows4, int B, int H, int W, void *stream);

/* layers.avg_pool(2) (scripts/models/layers.py:60-63), unfused form. */
int ssm_avgpool2_fwd(ssm_view x, ssm_view y, int B, int C, int H, int W, void *stream);

/* y = F.upsample(torch.cat([a, b], 1), size=(2h,2w), mode="bilinear")
 * (align_corners=False; scripts/models/flow_computation.py:244-245 and the
 * upsample lambdas :92-137).  Cb may be 0.  y is [B,Ca+Cb,2h,2w].            */
int ssm_upsample2x_cat_fwd(ssm_view a, int Ca, ssm_view b, int Cb, ssm_view y, int B, int h, int w,
                           void *stream);

/* layers.warp (scripts/models/layers.py:73-120): backward bilinear warp,
 * zeros outside, flow = (u,v).  img [B,C,H,W], flow [B,2,H,W], out [B,C,H,W].
 * This sampler and the entry points built on it below (ssm_flowinterp_inputs_fwd / _t_fwd, ssm_synthesize_fwd, the synthesis
 * fused into ssm_final_conv_fwd), together with ssm_avgpool2_fwd, ssm_upsample2x_cat_fwd, ssm_splitk_finish_fwd and
 * ssm_copy_view, are held to float64 references one by one, on contiguous tensors and on padded planes, at the sizes where
 * the 64 x 4 pixel blocks, an axis of one pixel and the image border decide the indexing:
 * tests/test_hip_infer_elementwise.py (references: tests/train_refs.py). */
int ssm_warp_bilinear_fwd(ssm_view img, ssm_view flow, ssm_view out, int B, int C, int H, int W,
                          void *stream);

/* FlowInterpolationModel.compute_inputs (scripts/models/flow_interpolation.py:
 * 338-372), fused: flow approximation + 2 warps + 16-channel concat.
 * img6 [B,6,H,W] (I0|I1), flow4 [B,4,H,W] (F01|F10), t[B] in (0,1) on device,
 * out16 [B,16,H,W] in the reference's channel order.                        */
int ssm_flowinterp_inputs_fwd(ssm_view img6, ssm_view flow4, const float *t, ssm_view out16, int B,
                              int H, int W, void *stream);
/* The same, writing only the ten t-dependent channels 3:13 of out16 (warped frames + approximated flows): for plans that convolve
 * the frame channels 0:3 / 13:16 (flow_interpolation.py:364-367) once per pair from the pair itself and never read them from out16
 * (ssm_amd.engine.UNetPlan.hoist) - 80 instead of 104 B/px of algorithmic traffic.                                              */
int ssm_flowinterp_inputs_t_fwd(ssm_view img6, ssm_view flow4, const float *t, ssm_view out16, int B, int H, int W, void *stream);

/* extract_outputs + compute_output_image (scripts/models/flow_interpolation.py:
 * 374-429), fused: sigmoid visibility, refined flows, 2 warps, blend.
 * y3 [B,3,H,W].  aux (ptr NULL = off) [B,5,H,W] receives Ft1(2) | Ft0(2) | V0(1),
 * the intermediates FullModel returns (scripts/models/superslomo_r.py:142-150). */
int ssm_synthesize_fwd(ssm_view img6, ssm_view in16, ssm_view out5, const float *t, ssm_view y3,
                       ssm_view aux, int B, int H, int W, void *stream);

/* Coarse-flow synthesis (beyond the reference's operator surface; an approximation of its output, not parity): the refined flows and
 * the visibility map come from a pass at 1/s of the frame's size, the frame is synthesised at full size from the original pixels.
 * img6 [B,6,H,W] full size (sb = 0: one pair for every entry), aux_lo [B,5,H/s,W/s] = Ft1(u,v) | Ft0(u,v) | V0 as ssm_synthesize_fwd
 * writes its `aux`, t[B] on the device, y3 [B,3,H,W].  s is 2 or 4, H = s*h, W = s*w; anything else is refused.  Per pixel (y, x):
 *   1. source position per axis as F.interpolate(scale_factor=s, mode="bilinear", align_corners=False):
 *      sy = max(0, (y + 0.5) / s - 0.5), i0 = floor(sy), i1 = min(i0 + 1, h - 1), lambda = sy - i0 (exact in fp32 for s = 2, 4);
 *   2. the five channels of aux_lo sampled bilinearly, columns first, then rows;
 *   3. both flows times s (pixels of the full-size frame); v0 = the sample of channel 4, v1 = 1 - v0;
 *   4. w0 = warp(I0, s*Ft0), w1 = warp(I1, s*Ft1) at full size: layers.warp (scripts/models/layers.py:100-119: normalise with
 *      max(size-1,1), grid_sample(align_corners=True), zeros outside), the device function ssm_synthesize_fwd uses;
 *   5. y = ((1-t)*v0*w0 + t*v1*w1) / ((1-t)*v0 + t*v1), grouped as scripts/models/flow_interpolation.py:420-427.
 * One fp32 operation per step, no contraction.                                                                          */
int ssm_synthesize_upscaled_fwd(ssm_view img6, ssm_view aux_lo, const float *t, ssm_view y3, int B, int H, int W, int s, void *stream);

/* Tiled inference (beyond the reference's operator surface; an approximation of the untiled output, not parity): the frames of one
 * tile are stitched into the full-size frames with a cross-fade over the seams.  tile [N,C,window_h,window_w] = the frames computed on
 * the window whose first pixel is canvas pixel (oy, ox); out [N,C,Hp,Wp].  The tile's core is rows [cy0, cy1) x columns [cx0, cx1) of the
 * canvas; `seams` = the sides of the core that have a neighbouring tile (bit 0 top, 1 bottom, 2 left, 3 right); b = 0 (hard seams) or a
 * power of two in 4..1024.  The call writes the tile's REGION OF INFLUENCE - the core grown by b across every side named in `seams`, cut
 * at the canvas - and no other element of `out`.  Per pixel (y, x) of it and per (n, c), v = the tile's value there:
 *   1. u(x; s) = clamp((x - s + b + 0.5) / (2b), 0, 1);  wx = (left ? u(x; cx0) : 1) * (right ? 1 - u(x; cx1) : 1), wy likewise from top
 *      / bottom / cy0 / cy1; b = 0: wx = wy = 1.  Every weight is an odd multiple of 1/(4b) or 0 or 1: all of this is exact in fp32,
 *      and the weights of the up to four tiles that reach a pixel sum to exactly 1;
 *   2. w = wy * wx, p = w * v;
 *   3. out = p where the pixel lies in neither the tile's left band (left and x < cx0 + b) nor its top band (top and y < cy0 + b),
 *      else out = out + p.
 * With the tiles of a grid stitched in RASTER ORDER on one stream, the tile of step 3's first case is the first to reach a pixel: `out`
 * needs no zero-fill and the result depends on nothing but that order.  One fp32 operation per step, no contraction: bit for bit
 * ssm_amd.tiles.stitch_host (tests/test_hip_tiles.py).  Refused: null pointers, a window or core outside the canvas, a window smaller
 * than the region of influence, a seam on a canvas edge, fade bands that meet (two opposite seams and 2b > core), any other b.
 * 16-byte accesses when both views are 16-byte aligned with strides of multiples of 4 and ox, cx0, cx1 and the region's columns are
 * multiples of 4 (the engine's grids: everything is a multiple of 32); one pixel per lane otherwise.  Measured (profiles/tiled_bench.txt):
 * the four launches that stitch a 2x2 tiling of 7 frames at 2176x3840 take 0.32 ms, 1.16x a device-to-device copy of the same bytes. */
int ssm_tile_stitch_fwd(ssm_view tile, ssm_view out, int N, int C, int window_h, int window_w, int Hp, int Wp, int oy, int ox, int cy0,
                        int cx0, int cy1, int cx1, int seams, int b, void *stream);

/* final_conv [+ synthesis]: Conv2d(32 -> NC, k3, pad 1, bias), no activation (scripts/models/flow_computation.py:145-153,
 * flow_interpolation.py:149-157), exact fp32: NC = 4 / 5 (the model's two filters) as v_fma_f32 chains in (cin, ky, kx) order,
 * every other NC (and $SSM_FINAL_VALU=0) on v_mfma_f32_4x4x1_16B_f32 (4 couts x 64 pixels per instruction).  x [B,32,H,W]
 * padded-plane view; w_oihw / bias the reference's state-dict tensors as they are (device fp32), NC <= 8.
 *   out (ptr NULL = off): [B,NC,H,W].
 *   y3 (ptr NULL = plain convolution): with NC = 5, extract_outputs + compute_output_image (flow_interpolation.py:374-429)
 *   run on the five sums in registers - arguments as ssm_synthesize_fwd, the 5-channel map is never written unless `out`
 *   is given too.                                                                                                       */
int ssm_final_conv_fwd(ssm_view x, const float *w_oihw, const float *bias, int NC, ssm_view out, ssm_view img6, ssm_view in16,
                       const float *t, ssm_view y3, ssm_view aux, int B, int H, int W, void *stream);

/* ---- launch programs (csrc/ssm_program.cpp) ------------------------------------------------------------------------
 * The reference's training loop (scripts/main.py:116-145,188-197) issues its step op by op through the framework; here a step is ~900
 * launches of this library with the SAME pointers, grids and arguments every time (the plans own every activation, gradient and packed
 * filter), so the host side of a step can be recorded once and replayed with a handful of calls (HIP graphs were measured slower than
 * eager issue on ROCm 7.2).
 *   ssm_program_create / destroy   a program handle
 *   ssm_program_begin   start recording with the pass's streams as slots 0..n-1 (n <= 8): from now on every launch of the library BY
 *                       THE CALLING THREAD is executed as usual AND appended to the program; launches of other host threads (the
 *                       reference's DataParallel replicas, scripts/main.py:74-76) run eagerly and stay out of it.  One recording at a
 *                       time per process: a second begin is refused (SSM_E_ARG, "another program is recording") - record later.  A
 *                       launch of the recording thread on a stream that is no slot makes ssm_program_end fail.
 *   ssm_program_mark    number of nodes recorded so far: a cut point for host-side work (framework kernels, collectives) that must run
 *                       between two ranges of nodes at replay
 *   ssm_program_end     stop recording; *n_nodes = nodes recorded
 *   ssm_program_run     issue nodes [first, last) again on `streams` (same count as at begin; normally the same handles); buffers
 *                       the recorded arguments point to must still be alive - they are the plans' own
 *   ssm_stream_wait     dst_stream waits for everything queued on src_stream so far (event record + wait).  The cross-stream ordering
 *                       of a pass (side stream of the weight gradients, VGG stream) must go through this call to be part of a program;
 *                       outside a recording it is a plain pair of HIP calls.                                                       */
int ssm_program_create(void **handle);
int ssm_program_destroy(void *handle);
int ssm_program_begin(void *handle, void *const *streams, int n_streams);
int ssm_program_mark(void *handle, int *n_nodes);
int ssm_program_end(void *handle, int *n_nodes);
int ssm_program_run(void *handle, int first, int last, void *const *streams, int n_streams);
int ssm_stream_wait(void *src_stream, void *dst_stream);

/* ---- frame formats either side of the path (uint8 HWC RGB on the device) ----------------
 * ssm_frames_from_u8_fwd: [N,H,W,3] uint8 -> normalised fp32 [N,3,Hp,Wp], image at (top,left),
 *   fusing ToTensor + Normalize + EvalPad (scripts/utils/dataloaders/augmentations.py:141-200;
 *   pad_before_norm=0: pad value 0 in normalised space) or the visualiser's load_batch +
 *   normalize_tensor (scripts/visualize_interpolation.py:61-88,257-262; pad_before_norm=1).
 *   mean3/std3 are HOST pointers to 3 floats (MODEL.PIXEL_MEAN / PIXEL_STD).
 * ssm_frames_to_u8_fwd: normalised fp32 [N,3,*,*] -> cropped [N,H,W,3] uint8: get_crop +
 *   denormalize + *255 + astype(uint8) (scripts/evaluate_interpolation_results.py:143-163,
 *   192-202).  mode 0 = the reference's cast (truncate, wrap mod 256); 1 = round + saturate. */
int ssm_frames_from_u8_fwd(const unsigned char *frames_hwc, ssm_view out, int N, int H, int W, int Hp, int Wp,
                           int top, int left, const float *mean3, const float *std3, int pad_before_norm,
                           void *stream);
int ssm_frames_to_u8_fwd(ssm_view in, unsigned char *frames_hwc, int N, int H, int W, int top, int left,
                         const float *mean3, const float *std3, int mode, void *stream);

/* ---- video frame formats (csrc/ssm_video.hip; planar Y'CbCr on the device, 8 to 16 bits per sample) ------
 * The streamed video loop (ssm_amd/video.py) serves the visualiser's convention, scripts/visualize_interpolation.py:
 * 61-88 (load_batch: frames padded to a multiple of 32, then normalised) and :223-268 (save_img_from_tensor,
 * normalize_tensor, denormalize), for frames that arrive as YUV4MPEG2 payloads instead of decoded RGB files.
 * A frame is the Y plane H x W, then U, then V, each ceil(H/2) x ceil(W/2) (SSM_YUV_420_*) or H x W (SSM_YUV_444),
 * rows unpadded; N frames are contiguous.  `table` is a HOST pointer to [2 matrices][2 ranges][SSM_YUV_ROW] floats,
 * built once in float64 and rounded to fp32 by ssm_amd.video.yuv_table(); row (matrix, range) holds
 *   [0..2] Kr Kg Kb    [3..6] rv = 2(1-Kr), gu = 2(1-Kb)Kb/Kg, gv = 2(1-Kr)Kr/Kg, bu = 2(1-Kb)
 *   [7..8] cbs = 1/(2(1-Kb)), crs = 1/(2(1-Kr))    [9..10] ys, cs = 255/219, 255/224 (limited) or 1, 1 (full)
 *   [11..12] iys, ics = 219/255, 224/255 or 1, 1    [13..14] yoff = 16 or 0, coff = 128
 *   [15..18] ylo yhi clo chi = 16 235 16 240 or 0 255 0 255    [19] 0
 * mean3 / std3 as for ssm_frames_from_u8_fwd.  Every operation below is one fp32 operation, rounded (no fused
 * multiply-add), in the order written.
 * ssm_frames_from_yuv_fwd: -> normalised fp32 [N,3,Hp,Wp] behind `out`, image at (top,left), pad value as
 *   ssm_frames_from_u8_fwd (pad_before_norm).  Per pixel (y,x):
 *     chroma: 4:4:4 c = C[y][x].  4:2:0, with i = y/2, j = x/2 and indices clamped to the plane:
 *       h(r, x even) = a0 C[r][j-1] + a1 C[r][j],   h(r, x odd) = b1 C[r][j] + b2 C[r][j+1]
 *       (a0 a1 b1 b2) = (.25 .75 .75 .25) SSM_YUV_420_CENTRED (420jpeg, 420), (0 1 .5 .5) SSM_YUV_420_COSITED (420mpeg2)
 *       c = .25 h(i-1) + .75 h(i) (y even),   .75 h(i) + .25 h(i+1) (y odd)
 *     y' = (Y - yoff) ys;  cb = (c_u - coff) cs;  cr = (c_v - coff) cs
 *     R = y' + rv cr;  G = (y' - gu cb) - gv cr;  B = y' + bu cb
 *     out = (min(max(v, 0), 255) / 255 - mean) / std   for v = R, G, B
 * ssm_frames_to_yuv_fwd: normalised fp32 [N,3,*,*] -> the H x W crop at (top,left) as N contiguous payloads.
 *   INPUTS MUST BE FINITE.  Per pixel: v = (in std + mean) 255 for R, G, B;
 *     Yf = (Kr R + Kg G) + Kb B;  Cb = (B - Yf) cbs;  Cr = (R - Yf) crs
 *     chroma sample (cy,cx) of 4:2:0, luma indices clamped to the crop:
 *       SSM_YUV_420_CENTRED  ((C[2cy][2cx] + C[2cy][2cx+1]) + (C[2cy+1][2cx] + C[2cy+1][2cx+1])) .25
 *       SSM_YUV_420_COSITED  h(r) = ((C[r][2cx-1] + 2 C[r][2cx]) + C[r][2cx+1]) .25;  (h(2cy) + h(2cy+1)) .5
 *     code = min(max(rint(Yf iys + yoff), ylo), yhi),   min(max(rint(C ics + coff), clo), chi)   (round half to even)
 * SSM_E_ARG for null pointers, N < 1 or > 65535, H or W < 1, a negative offset, a canvas smaller than the image
 * plus its offset, a row stride shorter than the canvas (ingest) or than left + W (egress), or a matrix, range
 * or siting outside the values below; SSM_YUV_422 is refused by these two entry points.
 *
 * ssm_frames_from_yuvx_fwd / ssm_frames_to_yuvx_fwd: the same two conversions for every layout below and for samples of
 * `sample_bytes` = 1 or 2.  A 2-byte sample is a 16-bit little-endian word with the value in its low bits (`bits` = 9 .. 16
 * significant ones: 420p10, 422p10, 444p12, ...), read and written as it stands; the payload pointer is then 2-byte
 * aligned (SSM_E_ARG otherwise; a frame has an even number of bytes, so every frame of a call is).  The kernels keep
 * working in 0 .. 255 units: the bit depth lives in `table` alone, ssm_amd.video.yuv_table(bits), where with s = 2^(bits-8)
 * and peak = 2^bits - 1
 *   limited: ys, cs = 255/(219 s), 255/(224 s); iys, ics = 219 s/255, 224 s/255; yoff, coff = 16 s, 128 s; bounds 16 s, 235 s, 16 s, 240 s
 *   full:    ys = cs = 255/peak; iys = ics = peak/255; yoff, coff = 0, 128 s; bounds 0, peak, 0, peak
 * (bits = 8 is the table above, bit for bit).  A word above peak is not refused: the clamp to [0, 255] bounds what it does.
 * SSM_YUV_422: chroma planes of H x ceil(W/2), co-sited with the even luma columns, no vertical step:
 *   ingest  c = h(y, x) of SSM_YUV_420_COSITED, (a0 a1 b1 b2) = (0 1 .5 .5), taken on row y of the chroma plane itself
 *   egress  C[y][cx] = ((C[y][2cx-1] + 2 C[y][2cx]) + C[y][2cx+1]) .25, columns clamped to the crop
 * With sample_bytes = 1 and a layout of the 8-bit entry points the result is theirs, bit for bit (they are this code).
 * SSM_E_ARG as above, and for a layout outside {0, 1, 2, 3}, sample_bytes outside {1, 2} or an odd address of 2-byte samples.
 *
 * Other matrices.  `matrix` is an index into the caller's table and stays within {0, 1}; the kernels read nothing of a matrix but its
 * row.  BT.2020 (non-constant luminance, Kr = 0.2627, Kb = 0.0593) comes as a table of its own, ssm_amd.video.yuv_table(bits,
 * BT2020): [1 matrix][2 ranges][SSM_YUV_ROW] of the same layout, built the same way, its rows at matrix index 0
 * (ssm_amd.video.table_index).  No Y4M header names the matrix: BT.2020 is the user's choice alone. */
#define SSM_YUV_ROW 20
#define SSM_YUV_BT601 0
#define SSM_YUV_BT709 1
#define SSM_YUV_LIMITED 0
#define SSM_YUV_FULL 1
#define SSM_YUV_420_CENTRED 0
#define SSM_YUV_420_COSITED 1
#define SSM_YUV_444 2
#define SSM_YUV_422 3
int ssm_frames_from_yuv_fwd(const unsigned char *frames_yuv, ssm_view out, int N, int H, int W, int Hp, int Wp,
                            int top, int left, const float *mean3, const float *std3, int pad_before_norm,
                            const float *table, int matrix, int range, int siting, void *stream);
int ssm_frames_to_yuv_fwd(ssm_view in, unsigned char *frames_yuv, int N, int H, int W, int top, int left,
                          const float *mean3, const float *std3, const float *table, int matrix, int range,
                          int siting, void *stream);
int ssm_frames_from_yuvx_fwd(const void *frames_yuv, ssm_view out, int N, int H, int W, int Hp, int Wp, int top, int left,
                             const float *mean3, const float *std3, int pad_before_norm, const float *table,
                             int matrix, int range, int layout, int sample_bytes, void *stream);
int ssm_frames_to_yuvx_fwd(ssm_view in, void *frames_yuv, int N, int H, int W, int top, int left, const float *mean3,
                           const float *std3, const float *table, int matrix, int range, int layout, int sample_bytes,
                           void *stream);

/* ---- shutter of the streamed video loop (csrc/ssm_video.hip; beyond the reference's operator surface) ----------------------------------
 * Definition (ssm_amd.video.Timeline(step, shutter=, samples=), everything in exact fractions).  `step` = input frames per output
 * frame, as without a shutter; shutter = sigma in (0, 1], the open fraction of the output interval (a shutter angle of 360 sigma
 * degrees); samples = S >= 1.  Output frame k is the mean of S sub-frames at
 *     tau(k, j) = k step + j d,   d = sigma step / S,   j = 0 .. S-1
 * - the shutter opens at the frame's own instant, so no sample lies before input frame 0.  With i = floor(tau), t = tau - i: t == 0 is
 * input frame i's ingested planes, anything else the frame synthesised between i and i + 1 at Timeline.t32(t).  Output k exists iff its
 * last sample does: tau(k, S-1) <= n - 1.  The mean is taken of the path's normalised fp32 planes - of the gamma-coded R'G'B' values, as a
 * frame-mixing filter does - or, through ssm_frames_accumulate_light_fwd below, of the light those values stand for.  S = 1 is the timeline without a shutter.  S = 8, the default of
 * the streamed loop, is a convention, not backed by a measurement of quality.
 * ssm_frames_accumulate_fwd: src [N,C,H,W], acc [1,C,H,W], both strided views (acc.sb is not read).  Per element, one rounded fp32
 * operation per step (no fused multiply-add), in this order:
 *   1. s = init ? src[0] : acc + src[0]
 *   2. s = s + src[n]   for n = 1 .. N-1, in increasing n
 *   3. acc = s * scale
 * bit for bit ssm_amd.video.accumulate_host (tests/test_hip_shutter.py).  A launch reads `acc` at most once (not at all with init = 1) and
 * writes it once, whatever N; nothing outside the H x W region of `acc` is written.  An output frame of the streamed loop is a chain of
 * such calls in time order on event-ordered streams: init = 1 on the first, scale = fp32(1 / S) on the last, 1 otherwise.
 * 16-byte accesses when both views are 16-byte aligned with strides of multiples of 4 and W % 4 == 0; one element per lane in the same
 * kernel otherwise.  No LDS, no scratch; no packed fp32 as the library is built (-fno-slp-vectorize in csrc/Makefile, fenced by
 * check_isa.sh: without that flag hipcc packs the four lanes of a 16-byte access into v_pk_add_f32 / v_pk_mul_f32).
 * SSM_E_ARG (nothing is launched) for null pointers; N, C, H or W < 1; N or C > 65535; H > 262140 (a lane group takes 4 rows and the
 * grid's y axis ends at 65535); a row stride shorter than W; init outside {0, 1}; a scale that is not finite; src and acc address ranges
 * that overlap. */
int ssm_frames_accumulate_fwd(ssm_view src, ssm_view acc, int N, int C, int H, int W, int init, float scale, void *stream);

/* ---- shutter in linear light (csrc/ssm_video.hip; beyond the reference's operator surface) ----------------------------------------------
 * A sensor integrates light, not code values: the mean of codes 0 and 255 is 128 on the codes and 188 in light under sRGB.  A light curve
 * maps a coded value c in [0, 1] to light L in [0, 1]; `curve` is a HOST pointer to one row of SSM_LIGHT_ROW floats, built in float64
 * and rounded once to fp32 by ssm_amd.video.light_curve(name) from the curve's (thr, slope, a, g):
 *   [0] thr  [1] 1/slope  [2] a  [3] 1/(1+a)  [4] g      decode(c) = c <= thr ? c * [1] : ((c + a) * [3]) ^ g
 *   [5] thr/slope  [6] slope  [7] 1+a  [8] 1/g           encode(L) = L <= [5] ? L * slope : [7] * L ^ [8] - a
 *   bt709   the inverse of the BT.709 camera curve (slope 4.5, exponent 0.45), with the two constants the standard prints to three digits
 *           (0.018, 1.099) taken to the digits at which its two pieces join in value and slope: scene light, what a shutter integrates
 *   srgb    0.04045, 12.92, 0.055, 2.4      bt1886   a pure power of 2.4 (thr = a = 0, slope = 1): the reference display with zero black
 * ssm_frames_accumulate_light_fwd: src [N,3,H,W], acc [1,3,H,W], strided views as for ssm_frames_accumulate_fwd; mean3 / std3 as for
 * ssm_frames_to_yuv_fwd.  Per element of plane p, in fp32, every operation rounded (no fused multiply-add), with
 *     dec(v) = v <= black[p] ? 0 : decode(min(max(v * std[p] + mean[p], 0), 1)),   black[p] = (0 / 255 - mean[p]) / std[p]
 *   - the egress kernel's denormalise, clamped, then the curve.  The comparison with the ingest kernels' black is the clamp's lower end
 *   said exactly: fp32 black * std + mean need not be 0 (the config's G plane gives 2^-25), and black must add no light.
 *   1. s = init ? dec(src[0]) : acc + dec(src[0])
 *   2. s = s + dec(src[n])   for n = 1 .. N-1, in increasing n
 *   3. r = s * scale
 *   4. acc = encode ? (encode(r) - mean[p]) / std[p] : r
 * x ^ e is 2 ^ (e * log2 x) by v_log_f32, one multiply and v_exp_f32 (1 ulp each by the ISA manual): the result is held to an error bound
 * against the float64 evaluation ssm_amd.video.accumulate_light_host, not to bits (tests/test_video_light_cpu.py derives the bound,
 * tests/test_hip_shutter_light.py asserts it).  Between an output's first call (init = 1) and its last (encode = 1, scale = fp32(1 / S))
 * the accumulator holds sums of light; after the last it holds normalised coded planes that ssm_frames_to_yuv_fwd reads unchanged.
 * The clamp is part of the definition: a synthesised value below 0 or above 1 counts as 0 or 1 before it is light, where the coded mean
 * of ssm_frames_accumulate_fwd lets it cancel against its neighbours in time.  Two properties hold exactly: a coded value <= 0 adds
 * exactly 0, and L = 0 encodes to exactly (0 - mean) / std, the ingest kernels' black, so a black region stays bit-identical black
 * through any number of samples.  INPUTS MUST BE FINITE.  Reads `acc` at most once, writes it once, nothing outside its H x W region;
 * access widths and the packed-fp32 fence as for ssm_frames_accumulate_fwd.
 * SSM_E_ARG (nothing is launched) for null pointers; N, H or W < 1; N > 65535; H > 262140; a row stride shorter than W; init or encode
 * outside {0, 1}; a scale, mean, std or curve constant that is not finite; a std that is not above 0; a curve row with g, 1/g, slope or 1/slope <= 0;
 * src and acc address ranges that overlap. */
#define SSM_LIGHT_ROW 9
int ssm_frames_accumulate_light_fwd(ssm_view src, ssm_view acc, int N, int H, int W, int init, float scale, const float *mean3,
                                    const float *std3, const float *curve, int encode, void *stream);

/* ---- shutter in the light of HDR clips: BT.2100 PQ and HLG (csrc/ssm_video.hip; beyond the reference's operator surface) ---------------
 * Camera material of 10 and 12 bits is BT.2020 with a PQ (SMPTE ST 2084) or HLG (ARIB STD-B67) transfer function; neither is a power law
 * with a linear toe, so they have an entry point and rows of their own.  Both act per channel on R'G'B' after the matrix, on c in [0, 1].
 * `consts` is a HOST pointer to one row of SSM_HDR_ROW floats, every one evaluated in float64 and rounded once to fp32 by
 * ssm_amd.video.hdr_light(name); `kind` says which of the two layouts it has.
 *   SSM_HDR_PQ   the BT.2100 PQ EOTF and its inverse; L in [0, 1] is DISPLAY light as a fraction of 10000 cd/m2 (no OOTF is applied):
 *       m1 = 2610/16384, m2 = 2523/4096 * 128, c1 = 3424/4096, c2 = 2413/4096 * 32, c3 = 2392/4096 * 32
 *       [0] 1/m2  [1] c1  [2] c2  [3] c3  [4] 1/m1     decode(c): p = c ^ [0];  L = (max(p - c1, 0) / (c2 - c3 * p)) ^ [4]
 *       [5] m1  [6] m2  [7] 0                          encode(L): y = L ^ m1;  c = L <= 0 ? 0 : ((c1 + c2 * y) / (1 + c3 * y)) ^ m2
 *     The formula at L = 0 gives c1 ^ m2 = 7.3e-7, one of the codes in [0, 7.3e-7] that all decode to L = 0 (p <= c1); of those, L <= 0
 *     encodes to 0: black comes back as black.
 *   SSM_HDR_HLG  the inverse of the BT.2100 HLG OETF and the OETF; E in [0, 1] is SCENE light, what a shutter integrates (no OOTF):
 *       a = 0.17883277, b = 1 - 4 a, cc = 0.5 - a ln(4 a)  (b and cc evaluated in float64 from a)
 *       [0] 1/3  [1] log2(e)/a  [2] cc  [3] b  [4] 1/12    decode(c) = c <= 1/2 ? (c * c) * [0] : (2 ^ ((c - cc) * [1]) + b) * [4]
 *       [5] a ln 2  [6] 0  [7] 0                           encode(E) = E <= [4] ? sqrt(3 * max(E, 0)) : [5] * log2(12 * E - b) + cc
 *     The two pieces meet in value and in slope at c = 1/2, E = 1/12; decode(1) = 1 to the digits of a.
 * ssm_frames_accumulate_hdr_fwd: ssm_frames_accumulate_light_fwd with these curves in place of its own - the same views, the same dec(v)
 * with its comparison against black, the same steps 1 to 4, the same kernel skeleton, access widths and launch geometry.  Every step
 * written above is one rounded fp32 operation (no fused multiply-add): x ^ e is 2 ^ (e * log2 x) by v_log_f32, a multiply and
 * v_exp_f32; n / d is n * v_rcp_f32(d), d within [0.16, 20]; sqrt is v_sqrt_f32; all four 1 ulp instructions by the ISA manual.  The result
 * is held to an error bound against the float64 evaluation ssm_amd.video.accumulate_hdr_host (tests/test_video_hdr_cpu.py derives it,
 * tests/test_hip_video_hdr.py asserts it).  Exact, as there: a coded value <= 0 adds exactly 0 (PQ: p = 0, no numerator; HLG: 0 * 0 / 3),
 * and L = 0 encodes to exactly (0 - mean) / std.  INPUTS MUST BE FINITE.
 * SSM_E_ARG (nothing is launched) for everything ssm_frames_accumulate_light_fwd refuses - null pointers (consts among them), the sizes,
 * a row stride shorter than W, init or encode outside {0, 1}, a scale, mean, std or constant that is not finite, a std that is not above
 * 0, overlapping address ranges - and for a kind outside the two below, a PQ row with an exponent or its reciprocal <= 0, c1 < 0, c3 < 0 or
 * c2 <= c3, an HLG row with [0], [1], [4] or [5] <= 0. */
#define SSM_HDR_ROW 8
#define SSM_HDR_PQ 0
#define SSM_HDR_HLG 1
int ssm_frames_accumulate_hdr_fwd(ssm_view src, ssm_view acc, int N, int H, int W, int init, float scale, const float *mean3,
                                  const float *std3, int kind, const float *consts, int encode, void *stream);

/* ---- shutter windows: weighted sub-frame sums (csrc/ssm_video.hip; beyond the reference's operator surface) ----------------------------
 * The three entry points above weigh every sub-frame alike (a box: scale = fp32(1 / S) on an output's last call).  A window gives sample
 * j of an output, at u_j = (j + 1/2) / S of the open interval, a weight w_j that falls off towards the ends of the exposure
 * (ssm_amd.video.shutter_window(name, S): triangle, hann, gauss[:K]; symmetric in j, so the blur's centre of mass stays where the box has
 * it) and closes the output with scale = fp32(1 / sum_j w_j), the sum of the fp32 weights taken in float64.
 * ssm_frames_accumulate_weighted_fwd, ssm_frames_accumulate_light_weighted_fwd, ssm_frames_accumulate_hdr_weighted_fwd: the sibling's
 * arguments, views, modes, dec and encode, and `weights`, a HOST pointer to N floats, weights[n] the weight of src[n] - for a call over the
 * samples j0 .. j0 + N - 1 of an output the slice w[j0 .. j0 + N - 1] of its window.  Per element, with p_n = weights[n] * dec(src[n])
 * (dec the identity in the coded form), every multiply and every add one rounded fp32 operation (no fused multiply-add), in this order:
 *   1. s = init ? p_0 : acc + p_0
 *   2. s = s + p_n   for n = 1 .. N-1, in increasing n
 *   3. r = s * scale
 *   4. acc = enc(r)   (coded: r; light and HDR: encode ? (encode(r) - mean[p]) / std[p] : r, as their siblings)
 * The coded form is bit for bit ssm_amd.video.accumulate_host(..., weights=) (tests/test_hip_shutter_window.py); with weights of 1 it is
 * bit for bit ssm_frames_accumulate_fwd (1 * x is x).  A sum issued in consecutive pieces - init on the first, scale and encode on the
 * last - is the same additions in the same order, so the same bits.  The light and HDR forms are held to bounds against the float64
 * yardsticks accumulate_light_host / accumulate_hdr_host(..., weights=), derived for weights in [0, 1] with scale * sum(weights) <= 1
 * in tests/test_video_window_cpu.py; their two exact properties stay: a coded value <= 0 adds w * 0 = 0, and black stays bit-identical black.
 * The weights travel by value in the kernel's arguments (SSM_ACC_WEIGHTS_MAX floats: no device buffer, no copy on the stream) and are read
 * as scalar operands; a longer sum is issued in pieces.  Access widths, launch geometry and the packed-fp32 fence as for the siblings.
 * SSM_E_ARG (nothing is launched) for everything the sibling refuses, and for a null `weights`, N > SSM_ACC_WEIGHTS_MAX, and a weight
 * that is not finite. */
#define SSM_ACC_WEIGHTS_MAX 64
int ssm_frames_accumulate_weighted_fwd(ssm_view src, ssm_view acc, int N, int C, int H, int W, int init, float scale,
                                       const float *weights, void *stream);
int ssm_frames_accumulate_light_weighted_fwd(ssm_view src, ssm_view acc, int N, int H, int W, int init, float scale, const float *weights,
                                             const float *mean3, const float *std3, const float *curve, int encode, void *stream);
int ssm_frames_accumulate_hdr_weighted_fwd(ssm_view src, ssm_view acc, int N, int H, int W, int init, float scale, const float *weights,
                                           const float *mean3, const float *std3, int kind, const float *consts, int encode, void *stream);

/* ---- scene cuts of the streamed video loop (csrc/ssm_video.hip; beyond the reference's operator surface) -------------------------------
 * Definition (ssm_amd.video.SceneCuts(threshold), everything in exact integers and fractions).  For the pair of input frames (i, i + 1)
 * of H x W pixels, with Y the 8-bit luma planes as they stand in the payloads:
 *     s = sum over the plane of |Y_i[y][x] - Y_(i+1)[y][x]|          (an integer, at most 255 H W)
 *     m = s / (H W);   score = min(m, |m - m_prev|) / 255;   the pair is a cut iff score >= threshold;   then m_prev = m
 * over the pairs in the order in which they run, m_prev = 0 before the first; a pair that a timeline skips is not fed.  The mean absolute
 * frame difference damped by its own change: steady fast motion has a large m and a small change.  A convention, not backed by a
 * measurement here; the threshold, a fraction in (0, 1], is the user's and has no default.  At a cut the streamed loop writes, for an
 * output at t < 1/2 between the two frames, the left frame's own bytes, for any other the right frame's.
 * ssm_luma_sad_fwd: a + n stride_a and b + n stride_b (strides in BYTES, of either sign) point at the Y planes of frames n = 0 .. N-1,
 * each H x W bytes with unpadded rows - a Y4M payload starts with its Y plane, so with stride = frame_bytes this addresses payloads
 * directly, whatever the chroma format.  sums[n] = s of (a_n, b_n), exact, in a device array of N 64-bit words.  The entry clears `sums`
 * on `stream` itself (a memset node ahead of the kernel): the result does not depend on what the words held.  a and b are only read and
 * may alias or overlap.  No byte outside the N planes of either operand is read.
 *   A workgroup of 256 lanes sums a span of 16 KiB of one plane: each lane 4 pieces of 16 bytes, 4 bytes per v_sad_u8 into a 32-bit lane
 *   sum (a span's sum is at most 255 * 16384 < 2^22), waves reduced by cross-lane shuffles, 4 wave partials through LDS, then one 64-bit
 *   vector atomicAdd into sums[n].  Integer adds commute: the sums are the same in every run.  One 16-byte load per operand and piece
 *   where both planes start on 16-byte boundaries; a plane that does not (odd frame sizes make n * frame_bytes odd), and the last piece
 *   of a plane whose size is no multiple of 16, goes through byte loads in the same kernel.  No LDS beyond the wave partials, no
 *   scratch, no packed fp32.  Reads 2 B per pixel.
 * SSM_E_ARG (nothing is queued) for null pointers; N outside 1..65535; H or W < 1; with N > 1 a |stride| shorter than H W; `sums` not
 * 8-byte aligned; a plane of more than 2^31 - 1 spans. */
int ssm_luma_sad_fwd(const unsigned char *a, const unsigned char *b, long long stride_a, long long stride_b, int N, int H, int W,
                     unsigned long long *sums, void *stream);

/* ---- hold-out scoring of the streamed video loop (csrc/ssm_video.hip; beyond the reference's operator surface) -------------------------
 * Definition (ssm_amd.video_score.HoldOutScorer(hold)).  Of a high-rate clip, input frames 0, hold, 2 hold, ... are KEPT and every frame
 * strictly between two kept ones is HELD OUT: frame i = g hold + k, 0 < k < hold, is synthesised at t = k / hold from kept frames g hold
 * and (g + 1) hold by the pipeline that the fixed grid of upsample_rate = hold runs, egressed to the clip's own format, and compared
 * with the held-out payload as it was read - the codes the tool would write, after quantisation ("model") - and the held-out payload is
 * compared with the nearer kept frame's, the left one for k / hold < 1/2 and the right one otherwise ("nearest", the do-nothing
 * baseline).  A comparison is, per plane p of Y, U, V:  sse_p = sum over the plane's samples of (a - b)^2, an integer;  mse = sse /
 * samples;  PSNR = 10 log10(peak^2 / mse) with peak = 2^bits - 1 whatever the code range (ffmpeg's `psnr` filter's convention), inf at
 * sse = 0.  Planes and frames are pooled by their sums: PSNR of (sum of sse) / (sum of samples), never a mean of dB.
 * ssm_plane_sse_fwd: a + n stride_a and b + n stride_b (strides in BYTES, of either sign, or 0: one payload against N) point at whole
 * Y4M payloads n = 0 .. N-1: the Y plane H x W, then U, then V, each of the layout's chroma size (SSM_YUV_420_*: ceil(H/2) x ceil(W/2),
 * SSM_YUV_422: H x ceil(W/2), SSM_YUV_444: H x W), unpadded.  sample_bytes = 1: bytes.  sample_bytes = 2: 16-bit little-endian words,
 * ALL 16 BITS COUNT (the bit depth does not enter).  sums[3 n + p] = sse_p of (a_n, b_n), exact, in a device array of 3 N 64-bit
 * words (exact while it is below 2^64: beyond 2^32 samples a plane).  The entry clears `sums` on `stream` itself (a memset node ahead of the kernel): the
 * result does not depend on what the words held.  a and b are only read and may alias or overlap.  No byte outside the N payloads of
 * either operand is read.
 *   A workgroup of 256 lanes sums a span of 16 KiB of ONE plane (the grid's x axis counts the Y plane's spans, then U's, then V's: no span
 *   crosses a plane boundary): each lane 4 pieces of 16 bytes.  Bytes: a.a + b.b - 2 a.b over four packed samples by three v_dot4_u32_u8,
 *   32-bit lane and workgroup sums (a span's sum is at most 65025 * 16384 < 2^30).  Words: (a - b)^2 reaches 2^32 - 131071, so the lane
 *   sum is 64-bit from the first add.  Waves reduced by cross-lane shuffles, 4 wave partials through LDS, one 64-bit vector atomicAdd per
 *   workgroup; integer adds commute: the sums are the same in every run.  One 16-byte load per operand and piece where both planes
 *   start on 16-byte boundaries; a plane that does not (odd H or W put U and V anywhere), and the last piece of a plane whose size is no
 *   multiple of a piece, goes sample by sample in the same kernel.  No LDS beyond the wave partials, no scratch, no packed fp32.  Reads
 *   2 sample_bytes per pair of samples, writes nothing but the sums.
 * SSM_E_ARG (nothing is queued) for null pointers; N outside 1..65535; H or W < 1; a layout outside SSM_YUV_*; sample_bytes outside
 * {1, 2}; a stride that is neither 0 nor at least the frame's bytes in magnitude; with sample_bytes = 2 an odd address or an odd stride;
 * `sums` not 8-byte aligned; a frame of more than 2^31 - 1 spans. */
int ssm_plane_sse_fwd(const void *a, const void *b, long long stride_a, long long stride_b, int N, int H, int W, int layout, int sample_bytes,
                      unsigned long long *sums, void *stream);

/* SSIM of the same comparisons, in fixed point (ssm_amd.video_score.plane_ssim_host is the definition in numpy).  The construction is that
 * of x264 and of ffmpeg's `ssim` filter.  Take a plane of rows x cols samples as it stands in the payload (row pitch cols, no padding):
 *   blocks   block (bx, by) is the 4 x 4 samples at (4 bx, 4 by), bx < cols >> 2, by < rows >> 2; the trailing cols & 3 columns and rows & 3
 *            rows belong to no block.  Per block  s1 = sum a,  s2 = sum b,  ss = sum (a^2 + b^2),  s12 = sum a b.
 *   windows  window (wx, wy) is the 8 x 8 area of blocks (wx .. wx + 1, wy .. wy + 1), at stride 4: it exists for wx < (cols >> 2) - 1 and
 *            wy < (rows >> 2) - 1;  count = max(0, (cols >> 2) - 1) max(0, (rows >> 2) - 1);  a plane of fewer than 8 rows or columns has
 *            none.  A window's four sums are the sums of its four blocks' sums.
 *   per window, in integers:  vars = 64 ss - s1^2 - s2^2;  covar = 64 s12 - s1 s2;
 *            f0 = 2 s1 s2 + c1;  f1 = 2 covar + c2;  f2 = s1^2 + s2^2 + c1;  f3 = vars + c2
 *            with c1 = floor(.01^2 peak^2 64 + .5), c2 = floor(.03^2 peak^2 64 63 + .5), peak = 2^bits - 1 of the clip's SIGNIFICANT bits
 *            (as in the PSNR, not the width of the word); the host passes c1 and c2 (ssm_amd.video_score.ssim_constants).  All four
 *            factors are below 2^45 at 16 bits and 2^29 at 8: exact in int64 and exact as doubles.
 *   in float64, one rounded operation each and no contraction:  q = (double(f0) double(f1)) / (double(f2) double(f3));
 *            fx = rint(q 2^32), half to even, as int64.
 *   result   sums[3 n + p] = sum over the windows of plane p (Y, U, V) of payload pair n of fx: a SIGNED 64-bit integer.  The SSIM of a
 *            plane is sums / (2^32 count); frames, positions and planes pool by sums and counts, as the PSNR does - "avg" is the sum over
 *            the planes of sums over 2^32 times the sum of their counts, pooled by WINDOWS, not ffmpeg's weighting by plane size; in dB,
 *            -10 log10(1 - ssim), inf at 1.
 * Fixed point makes the sum an integer: independent of the order of the atomics, the same in every run, and EQUAL to numpy's - which rests
 * on `/` of doubles being the correctly rounded IEEE quotient on the device (it is: the v_div_scale_f64 / v_rcp_f64 / v_fma_f64 /
 * v_div_fmas_f64 / v_div_fixup_f64 expansion, no fast-math flag in csrc/Makefile).
 * ssm_plane_ssim_fwd: a, b, the strides, N, H, W, layout and sample_bytes as for ssm_plane_sse_fwd; with sample_bytes = 2 all 16 bits of a
 * word enter the sums and the depth enters through c1 and c2 alone.  The entry clears the 3 N words of `sums` on `stream` itself, then the
 * kernel adds; a plane without a window keeps the cleared 0 (a frame without any window queues the clear alone).  a and b are only read
 * and may alias or overlap.  No byte outside the N payloads is read.
 *   A workgroup of 256 lanes owns a tile of 31 x 15 windows of ONE plane (the grid's x axis counts Y's tiles, then U's, then V's) and
 *   computes the 32 x 16 blocks under them, the last block column and row again in the neighbouring tile.  A lane takes two whole blocks:
 *   per row and operand one 4-byte word (bytes) or one 8-byte load (words) where plane start and cols make every row address aligned -
 *   decided per (n, plane) - and sample by sample otherwise, in the same kernel.  Bytes go through v_dot4_u32_u8 into 32-bit block sums;
 *   of words, ss and s12 are 64-bit from the first add.  Block sums go to LDS (8 or 12 KiB); after one barrier a lane forms two windows
 *   from four entries each, evaluates fx and adds to a 64-bit lane sum; shuffles, 4 wave partials through LDS, one 64-bit vector atomicAdd
 *   per workgroup.  No scratch, no packed fp32.
 * SSM_E_ARG (nothing is queued) as for ssm_plane_sse_fwd, under the name plane_ssim, and for c1 or c2 outside 1..2^40. */
int ssm_plane_ssim_fwd(const void *a, const void *b, long long stride_a, long long stride_b, int N, int H, int W, int layout, int sample_bytes,
                       long long c1, long long c2, long long *sums, void *stream);

/* The cross-fade of two payloads, the baseline `mix` of the hold-out score (what frame blending writes between two kept frames).
 * ssm_payload_mix_fwd: rows n = 0 .. N-1 of `samples` samples (bytes, or 16-bit little-endian words: sample_bytes = 1 or 2; planes need no
 * telling apart) at a + n stride_a, b + n stride_b (BYTES, either sign, or 0: one row for all n) and out + n stride_out.  With
 * k = num0 + n num_step every sample of row n is
 *     out = (a (den - k) + b k + (den >> 1)) / den          an integer division: the exact rational rounded half up
 * in 32-bit unsigned arithmetic (65535 * 65535 + 32767 < 2^32).  The division by the launch-constant den is Granlund and Montgomery's
 * multiply-shift with a host-computed pair, exact for every 32-bit numerator (csrc/ssm_video.hip; ssm_amd.video_score.mix_divisor is the
 * same pair, proven over the reachable numerators in tests/test_video_ssim_cpu.py).  16-byte loads and stores where the three rows of an n
 * start on 16-byte boundaries, sample by sample otherwise and at a row's end; nothing past `samples` is read or written.
 * SSM_E_ARG (nothing is queued) for null pointers; N outside 1..65535; samples < 1; sample_bytes outside {1, 2}; den outside 2..65535; a
 * k outside 0..den; a stride of a or b that is neither 0 nor at least the row's bytes; with N > 1 a |stride_out| shorter than the row;
 * with sample_bytes = 2 an odd address or stride; `out` overlapping a or b; a row of more than 2^31 - 1 spans of 16 KiB. */
int ssm_payload_mix_fwd(const void *a, const void *b, long long stride_a, long long stride_b, void *out, long long stride_out, int N,
                        long long samples, int sample_bytes, int num0, int num_step, int den, void *stream);

/* ---- interlaced clips of the streamed video loop (csrc/ssm_video.hip; beyond the reference's operator surface) -------------------------
 * Definition (ssm_amd.video.VideoInterpolator(deinterlace=); split_fields_host and weave_fields_host are the two entry points in numpy).
 * An interlaced frame of H x W weaves two FIELDS: in every plane the rows of parity 0 (0, 2, ...) are the TOP field's and the rows of parity 1
 * the BOTTOM field's - for SSM_YUV_420_* that includes the H/2-row chroma planes, chroma row r belongs to field r mod 2.  A field is
 * itself a payload of the frame's layout and sample size at H/2 x W, rows unpadded: its Y plane H/2 x W, then U, then V of the layout's
 * chroma size for H/2 rows.  H is even, and a multiple of 4 for SSM_YUV_420_*, so that both chroma fields have H/4 rows.  Field order
 * tff: frame m holds fields 2m (top, the earlier) and 2m + 1 (bottom) of the clip's 2n fields g_0 .. g_2n-1; bff: the bottom field is the
 * earlier one.  The output is 2n progressive frames: frame f has, in every plane, field g_f's bytes on the rows of g_f's parity; the other
 * rows are, for 0 < f < 2n - 1, those of the payload the fixed grid of upsample_rate = 2 writes at t = 1/2 between fields g_f-1 and
 * g_f+1 (same parity and line positions as the missing rows), and for f = 0 and f = 2n - 1 LINE AVERAGES of g_f itself: per plane a
 * missing row y is (a + b + 1) >> 1 per sample, in integers, a = kept row y - 1 and b = kept row y + 1 of the frame's plane; where one of
 * the two lies outside the plane, both are the other one.
 * ssm_fields_split_fwd: N contiguous frame payloads -> 2N contiguous field payloads, the top field of frame n at 2n and its bottom field
 * at 2n + 1: storage order is by row parity, not by time (the host maps field order to time).  Bytes are moved as they stand; a 2-byte
 * sample is moved whole, whatever its value.
 * ssm_fields_weave_fwd: output frame n (at frames + n stride_frames) takes its rows of parity (parity0 + n) & 1 from the field payload at
 * kept + n stride_kept; fill = 0: the other rows from the field payload at made + n stride_made; fill = 1: the other rows are the line
 * averages above of the kept field (`made` is not read and may be null).  Strides in BYTES of either sign; with N = 1 they name nothing.
 * kept and made are only read and may alias each other.
 *   Both kernels are one launch for the three planes: the grid's x axis counts 16-byte pieces of the frame's rows, Y's, then U's, then
 *   V's; a workgroup of 256 lanes takes 1024 of them, a lane 4, neighbouring lanes neighbouring pieces of a row; the grid's y axis is n.
 *   A piece is one 16-byte load (two for a line average) and one 16-byte store where it is whole and source and destination sit on
 *   16-byte boundaries, and moves sample by sample otherwise: a row's last piece when the row is no multiple of 16 bytes, rows that start
 *   anywhere (odd widths, a payload at an odd offset) - decided per piece, in the same kernel.  The average of packed samples is
 *   (a | b) - (((a ^ b) >> 1) & 0x7f7f7f7f) (0x7fff7fff for words).  No LDS, no scratch.  Each byte is read once (twice by a line average)
 *   and written once; nothing outside the payloads' rows is read or written.
 * SSM_E_ARG (nothing is queued), each with its own message and in this order: null pointers (made only with fill = 0); N outside
 * 1..65535; H or W < 1; a layout outside SSM_YUV_*; sample_bytes outside {1, 2}; an odd H; for SSM_YUV_420_* an H that is no multiple of
 * 4; a frame of more than 2^31 - 1 pieces; (weave) parity0 outside {0, 1}; fill outside {0, 1}; with sample_bytes = 2 an odd address,
 * (weave, N > 1) an odd stride; (weave, N > 1) a |stride| of kept or made shorter than a field, of frames shorter than a frame; an
 * output that overlaps an input. */
int ssm_fields_split_fwd(const void *frames, void *fields, int N, int H, int W, int layout, int sample_bytes, void *stream);
int ssm_fields_weave_fwd(const void *kept, long long stride_kept, const void *made, long long stride_made, void *frames, long long stride_frames,
                         int N, int H, int W, int layout, int sample_bytes, int parity0, int fill, void *stream);

/* ---- 3:2 pulldown removal of the streamed video loop (csrc/ssm_video.hip; beyond the reference's operator surface) ----------------------
 * Definition (ssm_amd.video.detelecine_host is all of it in numpy, Cadence the decision, TelecineSource the streamed form).  Film at 24
 * frames/s is carried in 30 frames/s video by 3:2 pulldown: four film frames A B C D become five video frames, fields as above (a frame's
 * top field T_n is the rows of parity 0 of every plane, its bottom field B_n the rows of parity 1).
 *   differences  per input frame n >= 1, over the LUMA plane only, two exact integers:
 *                dT[n] = sum |T_n - T_(n-1)|,  dB[n] = sum |B_n - B_(n-1)|.
 *   hypotheses   h = 5 pattern + phi, pattern in {0, 1}, phi in 0..4; frame n sits at cadence position q = (n - phi) mod 5, and the video
 *                frames are, as (top, bottom):
 *                    q            0       1       2       3       4
 *                    pattern 0  (A, A)  (B, B)  (B, C)  (C, D)  (D, D)      top field first: T repeats at q = 2, B at q = 4
 *                    pattern 1  (A, A)  (B, B)  (C, B)  (D, C)  (D, D)      bottom field first: B repeats at q = 2, T at q = 4
 *                No pattern-1 hypothesis shares both repeat positions with a pattern-0 one: the field order falls out of the data and the
 *                header's I tag is not looked at.
 *   windows      window j is frames 5 j + 1 .. 5 j + 5.  The score of h on it is dT[n2] + dB[n4] (pattern 0) or dB[n2] + dT[n4] (pattern 1),
 *                n2 and n4 the window's frames at q = 2 and q = 4.  The window takes the h of least score; on a tie at the minimum the
 *                previous window's h if it is among the tied ones, else the lowest h.  Frame 0 takes window 0's h; the frames after the
 *                last full window keep the last h.  A clip of fewer than 6 frames has no window and is refused.  There is no threshold: a
 *                convention, not backed by a measurement on compressed material; each window's (first frame, h, best, second-best score)
 *                is kept for the log.
 *   output       per frame n under its window's h:  q = 0, 1, 4: the frame's own bytes;  q = 2: nothing, the frame is dropped;  q = 3: a
 *                weave in EVERY plane, rows by parity - pattern 0: the top rows of frame n and the bottom rows of frame n - 1; pattern 1:
 *                the top rows of frame n - 1 and the bottom rows of frame n.  q = 3 at n = 0 has no predecessor: written as it stands.
 *                Every window holds exactly one q = 2 frame: four frames out per five in, rate (4 num, 5 den) reduced, 30000:1001 ->
 *                24000:1001, progressive.  H is even, a multiple of 4 for SSM_YUV_420_* (as for the interlaced clips above).
 * ssm_field_diff_fwd: a + n stride_a and b + n stride_b (strides in BYTES, of either sign, or 0: one plane against N) point at luma planes
 * n = 0 .. N-1 of H x W samples, rows unpadded.  sample_bytes = 1: bytes.  sample_bytes = 2: 16-bit little-endian words, ALL 16 BITS COUNT.
 *     sums[2 n + p] = sum over rows y = p (mod 2) of sum over x of |a_n[y][x] - b_n[y][x]|,   p = 0: the top fields, p = 1: the bottom fields
 * exact, in a device array of 2 N 64-bit words.  The entry clears them on `stream` itself (a memset node ahead of the kernel).  Odd H is
 * fine: parity 0 has one row more; with H = 1 the parity-1 word stays 0.  a and b are only read and may alias or overlap.  No byte outside
 * the N planes of either operand is read.
 *   The grid's x axis counts 16-byte pieces of the plane's rows, row by row (a row of W sample_bytes bytes has ceil of that / 16, the last
 *   one ragged); a workgroup of 256 lanes takes 1024 of them, a lane 4, 256 apart, neighbouring lanes neighbouring pieces of a row; the y
 *   axis is n.  Bytes go four per v_sad_u8, words two per v_sad_u16, into the 32-bit lane sum of the row's parity: a workgroup sees at
 *   most 16 KiB per operand, so every sum up to the workgroup's two is at most 65535 * 8192 < 2^29.  One 16-byte load per operand and piece
 *   where the piece is whole and both addresses sit on 16-byte boundaries, sample by sample otherwise and at a row's end, decided in the
 *   same kernel (uniformly for a workgroup where both planes and the row pitch are multiples of 16 bytes).  Waves reduced by cross-lane
 *   shuffles, 2 x 4 wave partials through LDS, then one 64-bit vector atomicAdd per parity and workgroup.  Integer adds commute: the sums
 *   are the same in every run.  No scratch, no packed fp32.  Reads 2 sample_bytes per pixel.
 * SSM_E_ARG (nothing is queued), each with its own message and in this order: null pointers; N outside 1..65535; H or W < 1; sample_bytes
 * outside {1, 2}; a stride that is neither 0 nor at least the plane's bytes in magnitude; with sample_bytes = 2 an odd address, then an
 * odd stride; `sums` not 8-byte aligned; a plane of more than 2^31 - 1 pieces. */
int ssm_field_diff_fwd(const void *a, const void *b, long long stride_a, long long stride_b, int N, int H, int W, int sample_bytes,
                       unsigned long long *sums, void *stream);

/* ---- field order from the data, for the interlaced clips of the streamed video loop (csrc/ssm_video.hip; beyond the reference's surface) --
 * Definition (ssm_amd.video.field_order_sums_host is all of it in numpy, field_kind the kind of a frame, FieldVerdict the decision over a
 * probe, FieldOrderSource the streamed form).  A Y4M header may say Ip or I? over interlaced material (ffmpeg writes Ip where it does not
 * know the order), and nothing refuses a wrong tff / bff: the fields are then woven in the wrong temporal order.  The operands are three
 * luma planes p, c, n - the frame before, the frame, the frame after - of H x W samples.  Everything is exact integers, over the rows
 * y = 1 .. H - 2 and all x:
 *     s[y][x] = c[y-1][x] + c[y+1][x]
 *     E_r[y]  = sum over x of |s[y][x] - 2 r[y][x]|          for r in {p, n, c}
 *     A0 = sum over even y of E_p[y] + sum over odd y of E_n[y]
 *     A1 = sum over odd y of E_p[y]  + sum over even y of E_n[y]
 *     D  = sum over y of E_c[y]
 *   why       under top-field-first an odd row of c lies half a frame AFTER its neighbours c[y +- 1]: row y of p is half a frame away from
 *             them and row y of n one and a half frames; for the even rows it is the other way round.  So A1 collects the near comparisons
 *             and A0 the far ones: tff gives A0 > A1, bff A1 > A0.  A progressive clip in motion gives A0 ~ A1 >> D, a still A0 = A1 = D.
 *             H < 3 has no such row: three zeros.
 *   kind      of a frame, in integers:  T if 25 A0 > 26 A1;  else B if 25 A1 > 26 A0;  else P if 2 min(A0, A1) > 3 D;  else U.
 *   verdict   over the kinds of frames 1 .. m - 2 of m probed frames, counts nT, nB, nP, nU and d = nT + nB + nP:  "tff" if 2 nT > d,
 *             "bff" if 2 nB > d, "progressive" if 2 nP > d, else none; fewer than 3 probed frames give none.
 *             The ratios 26/25 and 3/2 are conventions in the spirit of ffmpeg's idet, NOT its construction, and nothing here claims its
 *             decisions frame for frame; ffmpeg is not compared.  Not backed by a measurement on noisy or compressed footage.  A hard-edged
 *             shape that moves by whole rows biases one parity through its vertical edges: a progressive clip of one can come out B.
 * ssm_field_order_sums_fwd: p + i stride_p, c + i stride_c and n + i stride_n (strides in BYTES, of either sign, or 0) point at luma planes
 * i = 0 .. N-1 of H x W samples, rows unpadded.  sample_bytes = 1: bytes.  sample_bytes = 2: 16-bit little-endian words, ALL 16 BITS COUNT.
 *     sums[3 i + 0] = A0,  sums[3 i + 1] = A1,  sums[3 i + 2] = D          of (p_i, c_i, n_i)
 * exact, in a device array of 3 N 64-bit words.  The entry clears them on `stream` itself (a memset node ahead of the kernel; with H < 3
 * it is all that is queued).  Odd H and W = 1 are fine.  The operands are only read and may alias or overlap - frames i - 1, i, i + 1 of
 * one buffer are one pointer each and one stride.  No byte outside the N planes of an operand is read.
 *   The grid's x axis counts units: a unit is one 16-byte piece of the rows (a row of W sample_bytes bytes has ceil of that / 16, the last
 *   one ragged) over a band of 8 rows, bands from row 1 on; unit id is piece id mod pieces of band id / pieces, a workgroup of 256 lanes
 *   takes 256 of them, a lane one, neighbouring lanes neighbouring pieces of the same rows; the y axis is i.  A lane walks down its band
 *   with c[y-1], c[y], c[y+1] in registers.  Bytes are widened to pairs of packed 16-bit numbers (s <= 510) and go two per v_sad_u16,
 *   words one per 32-bit subtract.  |s - 2 r| <= 131070 per sample: a lane's three sums are at most 8 rows x 8 words x 131070 < 2^23
 *   each, a workgroup's 256 times that, 2147450880 < 2^31 - everything up to the workgroup's three sums fits 32 bits.  One 16-byte load
 *   per piece where it is whole and its address sits on a 16-byte boundary, sample by sample otherwise and at a row's end, decided in the
 *   same kernel (per lane without a test where the three planes and the row pitch are multiples of 16 bytes and the band is whole: all
 *   26 loads first).  Waves reduced by cross-lane shuffles, 3 x 4 wave partials through LDS, then one 64-bit vector atomicAdd per sum
 *   and workgroup.  Integer adds commute: the sums are the same in every run.  No scratch, no packed fp32.  Reads 3 sample_bytes per
 *   pixel and the two rows around a band of c again: 3.25.
 * SSM_E_ARG (nothing is queued), each with its own message and in this order: null pointers; N outside 1..65535; H or W < 1; sample_bytes
 * outside {1, 2}; a stride that is neither 0 nor at least the plane's bytes in magnitude; with sample_bytes = 2 an odd address, then an
 * odd stride; `sums` not 8-byte aligned; a plane of more than 2^31 - 1 pieces. */
int ssm_field_order_sums_fwd(const void *p, const void *c, const void *n, long long stride_p, long long stride_c, long long stride_n, int N,
                             int H, int W, int sample_bytes, unsigned long long *sums, void *stream);

/* ---- repeated frames of the streamed video loop (csrc/ssm_video.hip; beyond the reference's operator surface) ---------------------------
 * Definition (ssm_amd.video.dedup_host is all of it in numpy, Repeats the decision, RepeatSource and GapTimeline the streamed form).
 * Animation on twos or threes, 24 or 25 frames/s brought to 50 or 60 by repetition, screen recordings and captures that filled a dropped
 * frame hold frames that repeat the one before.  Everything below is in exact integers and fractions.
 *   blocks    a plane of rows x cols samples as it stands in a payload, rows unpadded: block (bx, by) is the 8 x 8 samples at (8 bx, 8 by),
 *             bx < cols >> 3, by < rows >> 3; the trailing cols & 7 columns and rows & 7 rows belong to no block (the rule of the SSIM
 *             blocks above), and a plane with fewer than 8 rows or columns has no block.  For payloads (a, b):
 *             d(block) = sum over the block of |a - b|; with 16-bit words all 16 bits count, d <= 64 * 65535 < 2^22.
 *   measure   per pair n and plane p (Y, U, V) over the plane's blocks:  max[n][p] = the largest d (0 for a plane without blocks),
 *             over[n][p] = the number of blocks with d > lo.  A small moving object cannot hide in it as it does in a whole-plane sum.
 *   test      frame n >= 1 is a REPEAT of frame n - 1 iff for every plane p that has blocks  max[n][p] <= hi  and
 *             over[n][p] <= floor(frac * blocks_p).  Frame 0 is never one.  The comparison is always with the frame directly before.
 *             Defaults hi = 768 * 2^(bits - 8), lo = 320 * 2^(bits - 8), frac = 33/100: the numbers of ffmpeg's mpdecimate (64 * 12,
 *             64 * 5, 0.33), NOT its construction - its blocks overlap at stride 4 and it counts against a quarter as many - so nothing
 *             here claims its decisions frame for frame; ffmpeg is not compared.  A convention, not backed by a measurement on compressed
 *             footage.  hi = lo = 0, frac = 0: exact repeats only.
 *   runs      a run is a maximal sequence of consecutive repeats, frames r + 1 .. r + m.  It is REPAIRED iff m <= D (dedup_max, default
 *             2: "on threes", 2:3 repetition) and frame r + m + 1 exists.  A longer run is a still, a run at the clip's end has no right
 *             neighbour: both stay as they are, every frame an ordinary input frame.
 *   output    the grid of upsample_rate N without the option: output k at input time k / N, k = 0 .. (n - 1) N.  For a repaired run
 *             frames r and r + m + 1 form ONE pair with gap g = m + 1; every output strictly between them, at input time r + j / N,
 *             j = 1 .. g N - 1, is the frame synthesised between r and r + m + 1 at t = j / (g N) (the engine's fp32 time: Timeline.t32).
 *             The repeats' own bytes are never written; the pairs inside the run do not run.  Every other frame at an integer time is
 *             its own bytes.  N = 1 is repair only.
 * ssm_block_sad_fwd: a + n stride_a and b + n stride_b (strides in BYTES, of either sign, or 0: one payload against N; rows n + 1 and n of
 * one buffer are fine) point at whole payloads n = 0 .. N-1 of H x W frames in `layout` (SSM_YUV_*), as for ssm_plane_sse_fwd.
 * sample_bytes = 1: bytes.  sample_bytes = 2: 16-bit little-endian words, ALL 16 BITS COUNT.
 *     out[6 n + 2 p] = max[n][p],   out[6 n + 2 p + 1] = over[n][p] with the given lo,   p = 0, 1, 2 for Y, U, V
 * exact, in a device array of 6 N 64-bit words.  The entry clears them on `stream` itself (a memset node ahead of the kernel).  a and b are
 * only read and may alias or overlap.  No byte outside the N payloads of either operand is read.
 *   A workgroup of 256 lanes owns a tile of 32 x 8 blocks of ONE plane, a lane one block; the grid's x axis counts Y's tiles (row-major),
 *   then U's, then V's, the y axis is n; a plane without a block has no tile, a frame without one no launch.  A lane loads the block's
 *   eight rows of both operands - bytes: one 8-byte load per row and operand, two v_sad_u8; words: one 16-byte load, four v_sad_u16 -
 *   into a 32-bit block sum; the 32 lanes of a tile row read neighbouring blocks.  The vector loads are used where the plane's start in
 *   both operands and its row pitch are multiples of the load (cols a multiple of 8), decided per (n, plane); otherwise the same kernel
 *   goes sample by sample (17 x 23 in 4:2:0 starts U at an odd byte).  Per-lane (d, d > lo) reduced by cross-lane shuffles, 2 x 4 wave
 *   partials through LDS, then ONE 64-bit vector atomicMax and ONE 64-bit vector atomicAdd per workgroup.  Both commute: the words are the
 *   same in every run.  No scratch, no packed fp32.  Reads 2 sample_bytes per sample of the blocks.
 * SSM_E_ARG (nothing is queued), each with its own message and in this order: null pointers; N outside 1..65535; H or W < 1; a layout
 * outside SSM_YUV_*; sample_bytes outside {1, 2}; a stride that is neither 0 nor at least the frame's bytes in magnitude; with
 * sample_bytes = 2 an odd address, then an odd stride; lo outside 0..2^22; `out` not 8-byte aligned; a frame of more than 2^31 - 1 tiles. */
int ssm_block_sad_fwd(const void *a, const void *b, long long stride_a, long long stride_b, int N, int H, int W, int layout, int sample_bytes,
                      int lo, unsigned long long *out, void *stream);

/* ---- blocks that do not change, of the streamed video loop (csrc/ssm_video.hip; beyond the reference's operator surface) -----------------
 * Definition (ssm_amd.video.static_paste_host is all of it in numpy).  A channel logo, burnt-in subtitles, the static parts of a screen
 * recording and a locked-off background are the same samples in both frames of a pair; synthesised, they come out re-quantised and pulled by
 * the flow of what moves beside them, and pulse against the input frames' own bytes.  Everything below is in exact integers.
 *   blocks    block (bx, by) of a FRAME is the 8 x 8 luma samples at (8 bx, 8 by), bx < W >> 3, by < H >> 3, together with the chroma samples
 *             under them, in U and in V: 4 x 4 at (4 bx, 4 by) for SSM_YUV_420_*, 8 rows x 4 columns at (4 bx, 8 by) for SSM_YUV_422, 8 x 8
 *             at (8 bx, 8 by) for SSM_YUV_444.  The trailing W & 7 columns and H & 7 rows, with the chroma under them, belong to no block
 *             (the rule of the blocks above); a frame with fewer than 8 rows or columns has none.
 *   measure   for the payloads (a, b) of a pair, d(block) = the sum of |a - b| over the block's luma, U and V samples; with 16-bit words
 *             all 16 bits count, d <= 192 * 65535 < 2^24.
 *   test      a block is STATIC in the pair iff d <= lo, lo an integer in 0 .. 2^24 - 1.  lo = 0: the two frames agree on every sample of
 *             the block.
 *   action    in every output strictly between the two frames the samples of a static block, luma and chroma, are the LEFT frame's (at
 *             lo = 0 the right frame's too); every other sample is what the run without the option writes.  Outputs that are input frames
 *             pass as their own bytes.
 *   count     per pair the number of static blocks.
 *   At lo = 0 this is no heuristic: where both neighbours hold the same samples no honest in-between frame differs.  NOT claimed: a block that
 *   agrees in both frames while something crossed it in between is kept (nothing can tell); seams between kept and synthesised blocks are
 *   not smoothed; a non-zero lo is the user's number, there is no default - the NUMBER in the spirit of mpdecimate's lo would be 320 at 8
 *   bits and is not backed by any measurement.
 * ssm_static_paste_fwd: a + n stride_a and b + n stride_b (strides in BYTES, of either sign; frames n and n + 1 of one buffer are fine; with
 * N = 1 they name nothing) point at the whole payloads of pair n = 0 .. N-1, H x W frames in `layout` (SSM_YUV_*), as for ssm_block_sad_fwd;
 * the T outputs of pair n are the payloads at out + (n T + j) stride_out, j < T (with N T = 1 the stride names nothing).  sample_bytes = 1:
 * bytes; 2: 16-bit little-endian words.  The outputs are read-modify-write: the only samples written are those of static blocks, which take
 * the samples of a_n; nothing outside the N T payloads is touched, a and b are only read and may alias or overlap each other.
 *     counts[n] = the number of static blocks of pair n
 * exact, N 64-bit words on the device, cleared by the entry itself on `stream` (a memset node ahead of the kernel).  A frame without blocks
 * queues the clear alone.
 *   A workgroup of 256 lanes owns a strip of 256 blocks of one pair, consecutive in row-major order, and takes them 32 at a time (grid:
 *   strips, n); 8 neighbouring lanes own a block, lane r of them its luma row r - bytes: one 8-byte load per operand, two v_sad_u8; words: one 16-byte load, four v_sad_u16 -
 *   and the chroma rows that fall to it: in 4:2:0 one row of 4 samples (U for r < 4, V above), in 4:2:2 row r of U and of V (4 samples), in
 *   4:4:4 row r of U and of V (8 samples), one load of 4, 8 or 16 bytes each.  A piece whose address does not sit on a boundary of its own
 *   size (odd widths, a payload at an odd offset) goes sample by sample, decided per piece in the same kernel.  The 8 lane sums are added by
 *   cross-lane shuffles, which leave d in all 8 lanes; where d <= lo every lane stores the pieces of `a` it loaded into the T outputs, by
 *   the same rule.  One flag per block, summed over the strip, through shuffles and LDS, then ONE 64-bit vector atomicAdd per workgroup.  Integer adds commute: the
 *   same words in every run.  Vector stores and vector atomics only; no scratch, no packed fp32.  Reads 2 sample_bytes per sample of the
 *   blocks, writes T sample_bytes per sample of the static ones.
 * SSM_E_ARG (nothing is queued), each with its own message and in this order: null pointers; N, then T, outside 1..65535; H or W < 1; a
 * layout outside SSM_YUV_*; sample_bytes outside {1, 2}; lo >= 2^24; with N > 1 a stride of a or b below the frame's bytes in magnitude; with
 * N T > 1 a |stride_out| below them; with sample_bytes = 2 an odd address, then an odd stride; `out` overlapping a or b; `counts` not 8-byte
 * aligned; a frame of more than 2^31 - 1 strips. */
int ssm_static_paste_fwd(const void *a, const void *b, long long stride_a, long long stride_b, void *out, long long stride_out, int N, int T,
                         int H, int W, int layout, int sample_bytes, unsigned int lo, unsigned long long *counts, void *stream);

/* ---- the flow check's per-block fallback, of the streamed video loop (csrc/ssm_video.hip; beyond the reference's operator surface) -------
 * Definition (ssm_amd.video.flow_paste_host is all of it in numpy).  The flow check scores a whole pair; one smeared object should not cost
 * the whole frame, and one bad region should not hide under a pair's score.  Everything below is in exact integers.
 *   blocks    the blocks of ssm_static_paste_fwd above: 8 x 8 luma samples at (8 bx, 8 by) with the chroma under them in U and V; the
 *             trailing W & 7 columns and H & 7 rows belong to no block, a frame with fewer than 8 rows or columns has none.
 *   measure   mask is what ssm_flow_consistency_fwd writes for the pair: uint8 [2][H][W], one plane per direction.  n(block) = the number
 *             of the block's 64 luma positions (y, x) at which bit 0 of mask[0][y][x] | mask[1][y][x] is set - for the bytes that kernel
 *             writes (0 consistent, 1 inconsistent, 2 leaves): inconsistent in at least one direction.  A pixel inconsistent in both
 *             directions counts once; a pixel that only leaves counts nothing.
 *   test      a block FAILS in the pair iff n > K, K an integer in 0 .. 64.  K = 64 fails nothing: the run without the option, byte for
 *             byte.  K = 0 fails every block that has one inconsistent pixel.
 *   action    in an output strictly between the two frames a failed block's samples, luma and chroma, are the NEARER input frame's: the
 *             left frame's at t < 1/2, the right frame's from there on - the rule of the cuts and of the pair-level fallback.  Every other
 *             sample is what the run without the option writes.  Outputs that are input frames pass as their own bytes.
 *   count     per pair the number of failed blocks.
 *   NOT claimed: K has no default; seams between pasted and synthesised blocks are not smoothed; a block from the nearer frame inside a
 *   moving region steps rather than moves; with this repository's synthetic weights nothing can be said about quality.
 * ssm_flow_paste_fwd: a + n stride_a and b + n stride_b (strides in BYTES, of either sign; frames n and n + 1 of one buffer are fine; with
 * N = 1 they name nothing) point at the whole payloads of pair n = 0 .. N-1, H x W frames in `layout` (SSM_YUV_*); pair n's two dense mask
 * planes are at mask + n stride_mask; its T outputs are the payloads at out + (n T + j) stride_out, j < T (with N T = 1 the stride names
 * nothing).  Outputs j < split take a_n's samples in failed blocks, outputs j >= split b_n's, 0 <= split <= T: the side is a launch scalar,
 * nothing is uploaded per call.  sample_bytes = 1: bytes; 2: 16-bit little-endian words.  The outputs are read-modify-write: the only
 * samples written are those of failed blocks; nothing outside the N T payloads is touched; a, b and mask are only read, and a and b may alias
 * or overlap each other.
 *     counts[n] = the number of failed blocks of pair n
 * exact, N 64-bit words on the device, cleared by the entry itself on `stream` (a memset node ahead of the kernel).  A frame without blocks
 * queues the clear alone.
 *   The skeleton is ssm_static_paste_fwd's: a workgroup of 256 lanes owns a strip of 256 blocks of one pair and takes them 32 at a time
 *   (grid: strips, n); 8 neighbouring lanes own a block, lane r of them luma row r and the chroma rows that fall to it.  Lane r loads its 8
 *   mask bytes of each direction - one 8-byte load where the address sits on an 8-byte boundary, byte by byte where not, decided per piece
 *   in the same kernel - ORs the two, keeps bit 0 of every byte and pop-counts; three cross-lane shuffles leave n in all 8 lanes.  Where
 *   n > K every lane loads its pieces of a (if split > 0) and of b (if split < T) and stores them into the outputs of that side, by the
 *   sibling's piece rule (4-, 8- or 16-byte accesses where aligned, sample by sample where not).  One flag per block, summed over the strip
 *   through shuffles and LDS, then ONE 64-bit vector atomicAdd per workgroup.  Vector stores and vector atomics only; no scratch, no
 *   floating point.  Reads 2 bytes of mask per luma sample and sample_bytes per sample and side of the failed blocks, writes T sample_bytes
 *   per sample of the failed ones.
 * SSM_E_ARG (nothing is queued), each with its own message and in this order: null pointers; N, then T, outside 1..65535; split outside
 * 0..T; H or W < 1; a layout outside SSM_YUV_*; sample_bytes outside {1, 2}; K outside 0..64; with N > 1 a stride of a or b below the
 * frame's bytes in magnitude; with N T > 1 a |stride_out| below them; with N > 1 a |stride_mask| below 2 H W; with sample_bytes = 2 an odd
 * address, then an odd stride; `out` overlapping a, b or mask; `counts` not 8-byte aligned; a frame of more than 2^31 - 1 strips. */
int ssm_flow_paste_fwd(const void *a, const void *b, long long stride_a, long long stride_b, void *out, long long stride_out, int N, int T,
                       int split, int H, int W, int layout, int sample_bytes, const unsigned char *mask, long long stride_mask, int K,
                       unsigned long long *counts, void *stream);

/* ---- the per-block fallback as a cross-fade, of the streamed video loop (csrc/ssm_video.hip; beyond the reference's operator surface) ------
 * Definition (ssm_amd.video.flow_mix_host is all of it in numpy and Python ints).  Inside a scene the nearer frame is the weakest fallback
 * there is: at eight outputs a pair a failed block shows the left frame four times and the right frame three times - it stands still and
 * then jumps while the picture around it moves.  A cross-fade of the two frames moves with it.  Everything below is in exact integers.
 *   blocks, measure, test, count   those of ssm_flow_paste_fwd above, word for word: n(block) > K fails, counts[n] the failed blocks.
 *   action    in output j of pair n every sample of a failed block, luma and chroma, is
 *                 (a (den - k_j) + b k_j + (den >> 1)) / den,   k_j = num0 + j num_step,   integer division,
 *             a and b the samples of a_n and b_n at its place: a (1 - t) + b t at the exact t_j = k_j / den, rounded half up.  Because it is
 *             the exact rational rounded half up, the value does not depend on which fraction names t: 2/5 and 400/1000 give the same
 *             bytes.  k_j = 0 gives a's samples, k_j = den gives b's.  16-bit words mix as words, all 16 bits; a mix of two codes <= 1023
 *             is <= 1023.  Every other sample is what the run without the option writes.
 *   NOT claimed: where the nearer frame steps, the cross-fade ghosts - both frames show through each other; which of the two looks better
 *   is not known, and with this repository's synthetic weights nothing can be said about quality; K has no default; seams between mixed and
 *   synthesised blocks are not smoothed.
 * ssm_flow_mix_fwd: a, b, out, mask, the strides, N, T, the frame and K as for ssm_flow_paste_fwd.  den in 2..65535 and every k_j, j < T, in
 * 0..den; the weights of output j are k_j and den - k_j, launch scalars: nothing is uploaded per call.  The numerator is at most
 * 65535 * 65535 + 32767 < 2^32; the division is ssm_payload_mix_fwd's multiply-shift, exact for every 32-bit numerator, its constants
 * computed on the host once per launch.  The outputs are read-modify-write: the only samples written are those of failed blocks; nothing
 * outside the N T payloads is touched; a, b and mask are only read, and a and b may alias or overlap each other.
 *     counts[n] = the number of failed blocks of pair n
 * exact, N 64-bit words on the device, cleared by the entry itself on `stream` (a memset node ahead of the kernel).  A frame without blocks
 * queues the clear alone.
 *   The skeleton and the measure are ssm_flow_paste_fwd's: strips of 256 blocks, 32 at a time, 8 neighbouring lanes a block, lane r of them
 *   luma row r and the chroma rows that fall to it; two 8-byte mask loads, OR, bit 0, pop-count, three cross-lane shuffles.  Where n > K
 *   a lane loads its pieces of a AND of b once and, per output, forms the mixed pieces word by word and stores them, by the sibling's piece
 *   rule (4-, 8- or 16-byte accesses where aligned, sample by sample where not).  ONE 64-bit vector atomicAdd per workgroup.  Vector loads,
 *   vector stores and vector atomics only; no scratch, no floating point.  Reads 2 bytes of mask per luma sample and 2 sample_bytes per
 *   sample of the failed blocks, writes T sample_bytes per sample of the failed ones.
 * SSM_E_ARG (nothing is queued), each with its own message and in this order: null pointers; N, then T, outside 1..65535; den outside
 * 2..65535; num0 or num0 + (T - 1) num_step outside 0..den (k_j is monotone in j: the two ends bound them all); then as
 * ssm_flow_paste_fwd from H or W < 1 on. */
int ssm_flow_mix_fwd(const void *a, const void *b, long long stride_a, long long stride_b, void *out, long long stride_out, int N, int T,
                     int num0, int num_step, int den, int H, int W, int layout, int sample_bytes, const unsigned char *mask,
                     long long stride_mask, int K, unsigned long long *counts, void *stream);

/* ---- letterboxed clips of the streamed video loop (csrc/ssm_video.hip; beyond the reference's operator surface) --------------------------
 * Definition (ssm_amd.video: active_counts_host, ActiveArea, cut_window_host and paste_window_host are all of it in numpy and Python ints,
 * ActiveSource the streamed form).  A 2.39:1 picture inside a 16:9 frame leaves bars that hold, at most, a subtitle or a logo.
 *   counts     rows[y] = the number of luma samples of row y whose value is above `limit`, cols[x] likewise of column x.  Chroma is not
 *              looked at; with 16-bit words all 16 bits count.
 *   lines      row y is ACTIVE in a frame iff rows[y] > frac * W, column x iff cols[x] > frac * H, compared exactly (integers against a
 *              fraction).  Defaults limit = 24 * 2^(bits - 8), frac = 1/64: 24 is the NUMBER of ffmpeg cropdetect's `limit`, NOT its
 *              construction (cropdetect averages a line), 1/64 is this project's own.  Conventions, not backed by a measurement on
 *              compressed footage, whose bars are noisy; every clip here is synthetic.
 *   rectangle  over the first P frames (active_probe, default 48; the whole clip if it is shorter) the smallest rectangle that holds every
 *              active row and column of every probed frame, aligned OUTWARD to (ay, ax) = (2, 2) for SSM_YUV_420_*, (1, 2) for
 *              SSM_YUV_422, (1, 1) for SSM_YUV_444: y0 and x0 multiples of it, the far edges multiples of it or the frame's own edge.
 *   fallback   the run is the one without the option, byte for byte, if the rectangle is the whole frame, no probed frame has an active
 *              row and column, or the rectangle is under 32 samples in a direction.
 *   window     the rectangle (w, h, x0, y0) of a payload as a payload of its own, a genuine h x w frame of the same layout: luma rows
 *              y0 .. y0 + h, columns x0 .. x0 + w; chroma rows y0 / ay .. ceil((y0 + h) / ay), columns x0 / ax .. ceil((x0 + w) / ax) with
 *              (ay, ax) the layout's subsampling - the planes of yuv_planes(h, w), since y0 and x0 are aligned.
 *   output     an output that coincides with an input frame is that frame's own bytes, whole.  A frame synthesised in pair (i, i + 1) at
 *              exact time t is, inside the rectangle, the frame the pipeline makes of the two cut windows - canvas, plan and launches of
 *              the cropped clip - and outside it the bytes of input i if t < 1/2, else of input i + 1: the rule of the scene cuts.
 * ssm_luma_counts_fwd: frames + n stride (stride in BYTES, of either sign; with N = 1 it names nothing) points at the luma plane of frame
 * n = 0 .. N-1, H x W samples, rows unpadded - a payload's first plane.  sample_bytes = 1: bytes; 2: 16-bit little-endian words.
 *     rows[n H + y], cols[n W + x] = the counts above, exact, 32-bit words in device arrays of N H and N W
 * Whatever the arrays held before, the call leaves them fully defined: the entry clears both on `stream` itself (two memset nodes ahead
 * of the kernel).  No byte outside the N planes is read.
 *   A workgroup of 256 lanes owns 256 columns x 32 rows of one frame (grid: column tiles, row bands, n): a lane four neighbouring columns -
 *   one 4- or 8-byte load where the plane's start and W are multiples of four samples (per n, uniform), sample by sample otherwise and
 *   never past a row's end - wave v of the four the rows v, v + 4, ... of the band.  Row counts: the lane's four flags, 64 lanes by
 *   cross-lane shuffles, one 32-bit vector atomicAdd per row and column tile.  Column counts: four lane counters over the wave's eight
 *   rows, the four waves' through LDS, one 32-bit vector atomicAdd per column and band.  Zero sums issue no atomic.  Integer adds
 *   commute: the words are the same in every run.  Vector atomics only; no scratch, no packed fp32.  Reads sample_bytes per pixel.
 * SSM_E_ARG (nothing is queued), each with its own message and in this order: null pointers; N outside 1..65535; H or W < 1; sample_bytes
 * outside {1, 2}; with N > 1 a stride below the plane's bytes in magnitude; with sample_bytes = 2 an odd address, then an odd stride;
 * limit outside 0..65535; rows or cols not 4-byte aligned; more than 65535 row bands (H > 2097120).
 * ssm_window_cut_fwd: frames + n stride_in points at whole payloads of H x W frames in `layout`, windows + n stride_out at the packed
 * windows of h x w at (y0, x0) that it writes (strides in BYTES, of either sign; with N = 1 they name nothing).  A byte mover: equal to
 * cut_window_host byte for byte, bytes or 16-bit words as they stand.  Nothing outside the window's samples is read, nothing outside the
 * N packed windows written.
 *   The walk of ssm_fields_split_fwd over the WINDOW's rows: 16-byte pieces, Y's rows, then U's, then V's, a lane 4 pieces 256 apart; a
 *   piece is one 16-byte load and store where it is whole and both addresses sit on 16-byte boundaries, sample by sample otherwise,
 *   decided per piece.  One launch for the three planes.  Reads and writes the window's bytes once each.
 * SSM_E_ARG (nothing is queued), in this order: null pointers; N outside 1..65535; H or W < 1; a layout outside SSM_YUV_*; sample_bytes
 * outside {1, 2}; a window that is empty or leaves the frame; one that is not aligned to the layout's (ay, ax) - the message names them;
 * a window of more than 2^31 - 1 pieces; with sample_bytes = 2 an odd address, then an odd stride; a stride below the frame's or the
 * window's bytes; windows overlapping frames. */
int ssm_luma_counts_fwd(const void *frames, long long stride, int N, int H, int W, int sample_bytes, int limit, unsigned *rows, unsigned *cols,
                        void *stream);
int ssm_window_cut_fwd(const void *frames, long long stride_in, void *windows, long long stride_out, int N, int H, int W, int y0, int x0, int h,
                       int w, int layout, int sample_bytes, void *stream);

/* ---- training ingest (csrc/ssm_data.hip; whole decoded uint8 HWC RGB frames on the device) --------------
 * The clip loader (ssm_amd/data.py) serves the reference's training transform, RandomCrop, then RandomMirrorRotate,
 * then Normalize and ToTensor (scripts/utils/dataloaders/default_reader.py:182-207,250-286, augmentations.py:
 * 39-92,181-200), for frames that arrive undecorated in one staging buffer: `frames` is that buffer on the device,
 * `frames_bytes` long, and sample b of the batch is described by record b of a table of B ssm_clip_record, which
 * the caller passes twice: `table_dev` on the device (normally the head of the same buffer, so that one copy moves
 * everything) and `table_host`, the host copy the argument checks read.  A sample's F frames, each hs x ws x 3
 * bytes, are contiguous from `offset` (bytes from `frames`); samples of one batch may differ in hs, ws.
 *   flags & SSM_CLIP_TRANSPOSE  the LOGICAL frame is the transpose of the stored one (the reference swaps the axes of
 *                               a stored frame with h > w): logical (y, x) = stored (x, y), h = ws, w = hs; else h = hs, w = ws
 *   (y1, x1)                    origin of the th x tw crop in the logical frame; crop pixel (y, x) = logical (y1 + y, x1 + x)
 *   flags & SSM_CLIP_HFLIP      the crop is mirrored: flipped crop pixel (y, x) = crop pixel (y, tw - 1 - x)
 *   flags & SSM_CLIP_AFFINE     the (flipped) crop is resampled through the inverse affine map a[0..5]
 * ssm_clip_batch_from_u8_fwd: frames 0 .. n_in - 1 of every sample -> `input`, contiguous fp32 [B, n_in, 3, th, tw];
 *   frames n_in .. F - 1 -> `target`, contiguous [B, F - n_in, 3, th, tw] (the tensors of Trainer.train_step with
 *   n_in = N_FRAMES, F = 2 N_FRAMES - 1; no padding).  With C the flipped crop of a frame as 8-bit values, per
 *   output pixel (y, x) and channel c, every operation one fp32 operation, rounded (no fused multiply-add), in the
 *   order written:
 *     integer mode (SSM_CLIP_AFFINE clear):  s = (float) C[y][x][c]
 *     affine mode:  u = (a[0] x + a[1] y) + a[2];  v = (a[3] x + a[4] y) + a[5]      (x, y as floats)
 *       i = floor(u), j = floor(v);  ax = u - i, ay = v - j;  bx = 1 - ax, by = 1 - ay
 *       top = C[j][i] bx + C[j][i+1] ax;  bot = C[j+1][i] bx + C[j+1][i+1] ax;  s = top by + bot ay
 *       with C = 0 outside [0,th) x [0,tw) (cv2.warpAffine's constant border, applied before normalisation; s = 0
 *       where u or v is not a number).  The host builds a[] in float64 as the inverse of cv2.getRotationMatrix2D(
 *       (cx, cy), theta, 1) and rounds it once to fp32; no transcendental runs on the device.  This is a stated
 *       definition, not cv2's fixed-point interpolation.
 *     out = (s / 255 - mean[c]) / std[c]          (the expression of ssm_frames_from_u8_fwd; mean3 / std3 as there)
 *   Integer mode is bit-equal to ssm_frames_from_u8_fwd of the host-cropped (and flipped) frames.
 * SSM_E_ARG (nothing is launched) for null pointers; B, F, th, tw or frames_bytes < 1; B F > 65535;
 * th ceil(tw / 4) > 2^31 - 1; n_in outside
 * 1 .. F - 1; and, read from table_host, a record with hs or ws < 1, a negative offset or an unknown flag, a
 * sample whose F frames leave the buffer, or a crop that leaves the logical frame (y1 < 0, x1 < 0, y1 + th > h,
 * x1 + tw > w). */
#define SSM_CLIP_TRANSPOSE 1
#define SSM_CLIP_HFLIP 2
#define SSM_CLIP_AFFINE 4
typedef struct {
    long long offset; /* bytes from `frames` to the sample's first frame */
    int hs, ws;       /* stored frame size */
    int flags;        /* SSM_CLIP_* */
    int y1, x1;       /* crop origin in the logical frame */
    float a[6];       /* inverse affine map (SSM_CLIP_AFFINE) */
    int reserved[3];  /* 0: records are 64 bytes */
} ssm_clip_record;
int ssm_clip_batch_from_u8_fwd(const unsigned char *frames, long long frames_bytes, const ssm_clip_record *table_dev,
                               const ssm_clip_record *table_host, float *input, float *target, int B, int F, int n_in,
                               int th, int tw, const float *mean3, const float *std3, void *stream);

/* ---- evaluator metrics of uint8 frames (an exception to the fp32-tensor convention: uint8 in, float64 out) ----
 * ssm_frame_metrics_fwd: per frame of two contiguous [N,H,W,3] uint8 stacks (what ssm_frames_to_u8_fwd
 *   writes) the sums behind Evaluator.eval_single_image (scripts/evaluate_interpolation_results.py:101-108:
 *   skimage's peak_signal_noise_ratio, structural_similarity(..., multichannel=True, gaussian_weights=True)
 *   and the interpolation error).  out is a DEVICE array [N][5] of float64:
 *     out[n][0] = SSE, the sum of squared differences over all H*W*3 values (an exact integer)
 *     out[n][1] = IE sum, sum over pixels of sqrt(sum_c d_c^2)
 *     out[n][2..4] = SSIM sum of channel 0, 1, 2 over the cropped interior [5,H-5) x [5,W-5): Gaussian
 *       sigma 1.5, 11 taps, scipy mode="reflect", sample covariance (121/120), K1 0.01, K2 0.03, range 255
 *   PSNR = 10 log10(255^2 / (SSE / (H*W*3))), SSIM = mean_c SSIM sum / ((H-10)(W-10)), IE = IE sum / (H*W).
 *   fp64 throughout; two launches, no atomics: bitwise repeatable, and frame n's sums do not depend on N.
 *   The workspace (device memory, ssm_frame_metrics_workspace_bytes(N, H, W) bytes at least) is the caller's.
 *   SSM_E_ARG for null pointers, N < 1, H or W < 11 (skimage's smallest image for its window) or a short
 *   workspace. */
size_t ssm_frame_metrics_workspace_bytes(int N, int H, int W);
int ssm_frame_metrics_fwd(const unsigned char *target_hwc, const unsigned char *output_hwc, int N, int H, int W,
                          void *workspace, size_t workspace_bytes, double *out, void *stream);

/* ---- optical-flow evaluation (csrc/ssm_flow.hip; fp32 flow in, float64 records / uint8 RGB out) -----------
 * Both entry points read `flow`, a planar fp32 [N,2,*,*] view (channel 0 = u, 1 = v; a 2-channel slice of
 * the 4-channel stage-1 output works through the view's strides), cropped at (top, left) to H x W: the crop of
 * scripts/evaluate_optical_flow_results.py:63-65 (rows 6:442 of the 448-row Sintel canvas).  Two launches each,
 * no atomics: bitwise repeatable, and field n's result does not depend on N, the stream or the run.  The
 * workspaces are device memory of the caller, *_workspace_bytes(N, H, W) bytes at least.
 *
 * ssm_flow_metrics_fwd: per field the sums behind compute_metrics (scripts/evaluate_optical_flow_results.py:
 *   18-28; mode 0: every pixel counts) or behind the convention of flow_error (scripts/utils/flo_utils.py:
 *   86-138; mode 1: pixels whose ground truth is unknown, |gt| > 1e7 in either component, or exactly zero in
 *   both components are left out).  gt_hw2: contiguous [N,H,W,2] fp32, the layout of a .flo payload, 8-byte
 *   aligned.  out is a DEVICE array [N][3] of float64:
 *     out[n][0] = sum over the counted pixels of sqrt(du^2 + dv^2), every operation of the per-pixel error
 *                 rounded to fp32 as numpy rounds it (no fused multiply-add), the sum in fp64
 *     out[n][1] = number of counted pixels whose error is > 3 (an exact integer)
 *     out[n][2] = number of counted pixels (an exact integer)
 *   EPE = out[0] / out[2], share of pixels more than 3 px off = out[1] / out[2].
 *   SSM_E_ARG for null pointers, N < 1 or > 65535, H or W < 1, a negative crop origin, a row stride shorter
 *   than left + W, a mode other than 0 / 1, a misaligned gt_hw2 or a short workspace.
 * ssm_flow_to_rgb_fwd: flow_to_image + compute_color + make_color_wheel (scripts/utils/flo_utils.py:141-272)
 *   per field -> contiguous [N,H,W,3] uint8 RGB.  Unknown pixels (|u| or |v| > 1e7) are flow 0 and black, NaN
 *   pixels black, as there.  Launch 1 reduces the field's maximum fp32 radius; launch 2 normalises by
 *   (double)maxrad + 2^-52 and evaluates the map in fp64 like the reference does on numpy >= 2, the radius
 *   un-fused so the `rad <= 1` branch is the reference's decision bit for bit; only atan2 may differ from
 *   numpy's in its last bits.  A field that holds a NaN is divided by -1 + 2^-52 instead of its maximum
 *   radius: np.max is NaN there and Python's max(-1, nan) returns -1 (flo_utils.py:166).
 *   SSM_E_ARG for null pointers, N < 1 or > 65535, H or W < 1, a negative crop origin, a row stride shorter
 *   than left + W or a short workspace. */
size_t ssm_flow_metrics_workspace_bytes(int N, int H, int W);
int ssm_flow_metrics_fwd(ssm_view flow, const float *gt_hw2, int N, int H, int W, int top, int left, int mode,
                         void *workspace, size_t workspace_bytes, double *out, void *stream);
size_t ssm_flow_to_rgb_workspace_bytes(int N, int H, int W);
int ssm_flow_to_rgb_fwd(ssm_view flow, unsigned char *rgb_hwc, int N, int H, int W, int top, int left,
                        void *workspace, size_t workspace_bytes, void *stream);

/* ---- forward-backward consistency of a pair's two flows (csrc/ssm_flow.hip) ----------------------------------
 * flow4: planar fp32 [N,4,*,*] as stage 1 leaves it, F01.u | F01.v | F10.u | F10.v, cropped at (top, left) to
 * H x W.  Where following one field and then the other does not lead back, the pixel is occluded or a flow is
 * wrong.  The definition, in fp32, one rounded operation per step, no fused multiply-add; F is one field
 * (planes u, v), G the other, (x, y) a pixel of the crop:
 *     u = F.u(y,x); v = F.v(y,x)
 *     px = (float)x + u;  py = (float)y + v
 *     leaves  iff  !(px >= 0 && px <= W-1 && py >= 0 && py <= H-1)              a NaN leaves
 *     x0 = floorf(px); y0 = floorf(py); fx = px - x0; fy = py - y0
 *     xi0 = (int)x0; xi1 = min(xi0 + 1, W-1); yi0, yi1 likewise                  only taps inside the crop are read
 *     for each plane g of G:  a = g(yi0,xi0) + fx * (g(yi0,xi1) - g(yi0,xi0))
 *                             b = g(yi1,xi0) + fx * (g(yi1,xi1) - g(yi1,xi0))
 *                             g' = a + fy * (b - a)
 *     rx = u + u'; ry = v + v'
 *     e2 = rx*rx + ry*ry
 *     m2 = ((u*u + v*v) + u'*u') + v'*v'
 *     inconsistent  iff  e2 > alpha * m2 + beta                                  judged pixels only; strict
 *     residual = sqrtf(e2)                                                       correctly rounded
 *   Direction 0 is F = F01, G = F10; direction 1 the roles swapped.  alpha = 0.01 and beta = 0.5 are the numbers
 *   of Sundaram, Brox and Keutzer (2010) as most later work uses them: a convention, not backed by a measurement
 *   here, and no default of this entry point.
 *   out is a DEVICE array [N][2][4] of float64, per pair and direction:
 *     [0] judged: pixels that do not leave    [1] inconsistent    [2] leaves          (exact integers)
 *     [3] the sum of the judged pixels' residuals, in fp64
 *   mask (DEVICE, or null): uint8 [N][2][H][W], 0 consistent, 1 inconsistent, 2 leaves.
 *   Both directions in one launch, a second sums the workgroups' slots: no atomics, bitwise repeatable, pair n's
 *   result does not depend on N, the stream or the run.  Nothing outside the crop is read.  The workspace is
 *   device memory of the caller, ssm_flow_consistency_workspace_bytes(N, H, W) bytes at least, 8-byte aligned.
 *   SSM_E_ARG for null pointers (the view's, workspace, out), N < 1 or > 65535, H or W < 1, a negative crop
 *   origin, a row stride shorter than left + W, a misaligned workspace or out. */
size_t ssm_flow_consistency_workspace_bytes(int N, int H, int W);
int ssm_flow_consistency_fwd(ssm_view flow4, int N, int H, int W, int top, int left, float alpha, float beta,
                             void *workspace, double *out, unsigned char *mask, void *stream);

/* ---- backward kernels of the training step (fp32 planes; BASELINE config 3) ------------------------------
 * The data gradient of a convolution is ssm_conv2d_fwd on the transposed, spatially flipped filter.
 * ssm_lrelu_bwd           dz = (dy + 1/4 dpool[y/2][x/2]) * (y > 0 ? 1 : slope)   (dy or dpool may be NULL views;
 *                         has_act = 0 for the bare final_conv)  - LeakyReLU' + adjoint of the fused 2x2 mean
 * ssm_bias_grad           db[c] = sum dz
 * ssm_conv2d_wgrad        dw[:, ci_offset:ci_offset+Cin] of an OIHW fp32 filter with cin_total inputs (zeroed first if
 *                         zero_first; two-source convs call it once per source) += sum_{b,y,x} dz * x(shifted); x padded planes
 * ssm_upsample2x_cat_bwd  adjoint of ssm_upsample2x_cat_fwd; acc_a/acc_b: add into da/db instead of overwriting
 * ssm_synthesize_bwd      adjoint of ssm_synthesize_fwd fused with d(L1 reconstruction) and, if stage2_terms, the two
 *                         refined-flow warp-loss terms (scripts/models/losses.py:160-161,217); c_rec[b], c_warp[b] =
 *                         lambda * upstream gradient / (3*H*W) per sample (device arrays); est4 = Ft1^ | Ft0^;
 *                         dy_extra (NULL view = none): gradient of further loss terms wrt the frame (the perceptual term)
 * ssm_flowinterp_inputs_bwd  adjoint of ssm_flowinterp_inputs_fwd wrt the stage-1 flows, fused with the two stage-1
 *                         warp-loss terms (losses.py:152-154) if stage1_terms                                   */
/* Adjoint of ssm_warp_bilinear_fwd (autograd of layers.warp, scripts/models/layers.py:73-120, as used by the loss terms
 * scripts/models/losses.py:152-161): dflow [B,2,H,W] (NULL view = not wanted) and dimg [B,C,H,W] (NULL view = not wanted;
 * ACCUMULATED into with atomics - zero it first - and it must share img's row stride).                                 */
int ssm_warp_bilinear_bwd(ssm_view img, ssm_view flow, ssm_view dy, ssm_view dflow, ssm_view dimg, int B, int C, int H, int W,
                          void *stream);
int ssm_lrelu_bwd(ssm_view dy, ssm_view dpool, ssm_view y, ssm_view dz, int B, int C, int H, int W, float slope, int has_act,
                  void *stream);
/* ssm_lrelu_bwd that also writes dZ in the Q8 operand form (dz_q8: an even number of channel groups >= ceil(C/8), zero-initialised
 * beyond C) - the input of the data-gradient convolution when the training step runs the fp16 + fp8 kernels.               */
int ssm_lrelu_bwd_q8(ssm_view dy, ssm_view dpool, ssm_view y, ssm_view dz, ssm_hview dz_q8, int B, int C, int H, int W, float slope,
                     int has_act, void *stream);
int ssm_bias_grad(ssm_view dz, float *db, int B, int C, int H, int W, void *stream);
/* db[c] += sum dz (no zeroing): the training step zeroes one flat buffer holding every parameter gradient of a U-Net once. */
int ssm_bias_grad_acc(ssm_view dz, float *db, int B, int C, int H, int W, void *stream);
int ssm_conv2d_wgrad(ssm_view x, ssm_view dz, float *dw_oihw, int B, int Cin, int Cout, int H, int W, int k, int cin_total,
                     int ci_offset, int zero_first, void *stream);
/* ssm_conv2d_wgrad that also ACCUMULATES the bias gradient db_acc[co] += sum_{b,y,x} dz (what autograd computes for nn.Conv2d.bias,
 * scripts/models/layers.py:21-33): the sum over pixels is one more column of the same GEMM (dZ times a row of ones), so the separate
 * ssm_bias_grad pass over dZ - 48 launches of a training step - disappears.  Call it for ONE of a two-source layer's sources.        */
int ssm_conv2d_wgrad_bias(ssm_view x, ssm_view dz, float *dw_oihw, float *db_acc, int B, int Cin, int Cout, int H, int W, int k,
                          int cin_total, int ci_offset, int zero_first, void *stream);
/* Same contract as ssm_conv2d_wgrad (what autograd computes for nn.Conv2d.weight, scripts/models/layers.py:21-33 trained by
 * scripts/main.py:138-197) on the bf16 matrix cores with split operands: v = bf16(v) + bf16(v - bf16(v)) + r, products
 * hi*hi + hi*lo + lo*hi accumulated in fp32 (dropped terms ~2^-17 relative; no scaling needed, bf16 has fp32's exponent).
 * The weight gradient of the f16f8 training plan; the exact-fp32 plan keeps ssm_conv2d_wgrad.                                 */
int ssm_conv2d_wgrad_bf16x3(ssm_view x, ssm_view dz, float *dw_oihw, int B, int Cin, int Cout, int H, int W, int k, int cin_total,
                            int ci_offset, int zero_first, void *stream);
/* Weight gradient of a 3x3 layer in the Winograd domain, F(2x2,3x3), fp32 throughout (csrc/ssm_wgradw.hip) - the same quantity as
 * ssm_conv2d_wgrad(k = 3) (autograd of nn.Conv2d.weight, scripts/models/layers.py:21-33 under scripts/main.py:138-197) for 16 instead of
 * 36 multiplies per 2x2 output tile, in two launches:
 *   ssm_conv2d_wgrad_wino   du[16][Cout][cin_total] (+ ci_offset) += sum_tiles (A dZ A^T) (.) (B^T x B)     fp32 atomics; du must be
 *                           zero before a step's first launch (ssm_wgrad_wino_scratch_floats floats; the finishing launch re-zeroes
 *                           it); db_acc (may be NULL): += sum dz, as ssm_conv2d_wgrad_bias; two-source layers call it once per source
 *   ssm_wgrad_wino_finish   for each job: dw_oihw[co][ci][3][3] += scale * G^T du[.][co][ci] G, du := 0.  `jobs` is a DEVICE array of
 *                           n_jobs ssm_wgradw_finish_job records (one per layer: a training step finishes a gradient bucket's layers
 *                           in one launch); max_n = the largest n among them
 * ssm_wgrad_wino_supported: 3x3, Cin and Cout >= 32, maps of 40+ pixels (below that K = tiles is too short against the 16 x Cout x
 * Cin partial sums every workgroup adds; those layers keep ssm_conv2d_wgrad).                                                      */
typedef struct ssm_wgradw_finish_job {
    float *du;       /* [16][Cout][cin_total] scratch of the layer                 */
    float *dw;       /* [Cout][cin_total][3][3] gradient, accumulated into         */
    int n;           /* Cout * cin_total                                           */
    int pad_;
} ssm_wgradw_finish_job;
int ssm_wgrad_wino_supported(int Cin, int Cout, int H, int W, int k);
long long ssm_wgrad_wino_scratch_floats(int Cout, int cin_total);
int ssm_conv2d_wgrad_wino(ssm_view x, ssm_view dz, float *du, float *db_acc, int B, int Cin, int Cout, int H, int W, int cin_total,
                          int ci_offset, void *stream);
int ssm_wgrad_wino_finish(const void *jobs_dev, int n_jobs, int max_n, float scale, void *stream);
int ssm_upsample2x_cat_bwd(ssm_view du, ssm_view da, int Ca, ssm_view db, int Cb, int B, int h, int w, int acc_a, int acc_b,
                           void *stream);
/* ... with the LeakyReLU' of the layer that produced `a` applied to da (after the optional accumulation): da = dZ of that layer, ya = its
 * output [B, Ca, h, w] - the a-source of a decoder level has no other consumer (scripts/models/flow_computation.py:244-247).               */
int ssm_upsample2x_cat_bwd_mask(ssm_view du, ssm_view da, int Ca, ssm_view db, int Cb, ssm_view ya, float slope, int B, int h, int w,
                                int acc_a, int acc_b, void *stream);
int ssm_synthesize_bwd(ssm_view img6, ssm_view est4, ssm_view out5, ssm_view target, const float *t, const float *c_rec,
                       const float *c_warp, ssm_view dy_extra, ssm_view dout5, ssm_view dest4, int B, int H, int W, int stage2_terms,
                       void *stream);
int ssm_flowinterp_inputs_bwd(ssm_view img6, ssm_view flow4, ssm_view din16, ssm_view dest4, const float *t, const float *c_warp,
                              ssm_view dflow4, int B, int H, int W, int stage1_terms, void *stream);

/* ---- perceptual loss (PerceptualLoss: vgg16.features[:23] + MSELoss, scripts/models/losses.py:12-41,172-181,218-233) --
 * The VGG convolutions are ssm_conv2d_fwd launches with SSM_FLAG_LRELU and slope 0 (= ReLU); their data gradients are the
 * same kernel on the transposed filters, ReLU' is ssm_lrelu_bwd with slope 0.  fp32 planes.
 *  ssm_maxpool2_fwd   y[B,C,H/2,W/2] = nn.MaxPool2d(2, 2)(x)                       (H, W = input size, even)
 *  ssm_maxpool2_bwd   dx = dy routed to the first maximum of each 2x2 window (row-major scan, as torch's backward)
 *  ssm_sqdiff_grad    out = coef[b] * (a - b): gradient of the per-sample mean squared feature difference
 *  ssm_sqdiff_mean    out[b] = mean over C x H x W of (a - b)^2, the per-sample MSELoss(reduce=False).mean of losses.py:218,227
 *                     (two deterministic launches; scratch: 64 * B device floats owned by the caller)                    */
int ssm_maxpool2_fwd(ssm_view x, ssm_view y, int B, int C, int H, int W, void *stream);
int ssm_maxpool2_bwd(ssm_view x, ssm_view dy, ssm_view dx, int B, int C, int H, int W, void *stream);
int ssm_sqdiff_grad(ssm_view a, ssm_view b, const float *coef, ssm_view out, int B, int C, int H, int W, void *stream);
int ssm_sqdiff_mean(ssm_view a, ssm_view b, float *scratch, float *out, int B, int C, int H, int W, void *stream);
/* The L1 terms of SSMLosses.forward (scripts/models/losses.py:113-170 warp terms with the FREEZE gating of :159-167, :218-233
 * reconstruction) of one window as per-sample sums, out[b][0] = sum |pred - target|, out[b][1] = sum of the (up to four) warp maps -
 * the caller divides by 3 H W and applies lambda_r / lambda_w.  img6 = [I0 | I1], flow4 = stage 1's [F01 | F10], est4 = the approximated
 * flows [Ft1 | Ft0] (channels 6:10 of the stage-2 input), out5 = stage 2's output, pred = the synthesised frame.  Two deterministic
 * launches; scratch: 128 * B device floats owned by the caller.                                                                     */
int ssm_train_loss_sums(ssm_view img6, ssm_view flow4, ssm_view est4, ssm_view out5, ssm_view pred, ssm_view target, float *scratch,
                        float *out, int B, int H, int W, int stage1_terms, int stage2_terms, void *stream);

/* ---- recurrent bottleneck (BOTTLENECK=CLSTM|CGRU; BASELINE config 4) -----------------------------------------
 * Replaces ConvBLSTM / ConvBGRU(in_channels=512, hidden_channels=512, kernel_size=(3,3), num_layers=2,
 * batch_first=True) as constructed at scripts/models/flow_computation.py:73-88 / flow_interpolation.py:73-88 and
 * called at flow_computation.py:208-211 / flow_interpolation.py:284-287 (`conv6(x_fwd, x_rev)`).  Their source is
 * an un-vendored submodule (.gitmodules:1-3, SreenivasVRao/ConvGRU-ConvLSTM-PyTorch, commit not recorded); the
 * cells below restate that package's published equations - parity UNPINNED.
 * The gate convolutions are ssm_conv2d_fwd / ssm_conv2d_hl8_fwd launches without activation: `gates_x` = the
 * filter's input-channel part applied to x_t (+ bias; batched over the sequence), `gates_h` = its hidden-channel
 * part applied to h_{t-1} (NULL view at the first step: h_0 = c_0 = 0).  All tensors [B,*,H,W]; Hc % 8 == 0.
 * Outputs go to fp32 planes (h_f32) and/or an HL8 view (h_hl8), either may be a NULL view.
 *  ssm_convlstm_cell_fwd   gates [i|f|o|g] (4*Hc ch): c' = s(f)*c + s(i)*tanh(g);  h' = s(o)*tanh(c')
 *  ssm_convgru_reset_fwd   gates [gamma|beta] (2*Hc ch): rh = s(gamma) * h          (input of the candidate conv)
 *  ssm_convgru_update_fwd  u = s(beta); h' = (1-u)*h + u*tanh(cand_x + cand_h)      (cand_* = Hc ch)            */
/* flags: SSM_FLAG_Q8 = write the HL8 output in the Q8 operand form (view starting at an even channel group, Hc % 16 == 0) */
int ssm_convlstm_cell_fwd(ssm_view gates_x, ssm_view gates_h, ssm_view c_prev, ssm_view c_next, ssm_view h_f32,
                          ssm_hview h_hl8, int B, int Hc, int H, int W, int flags, void *stream);
int ssm_convgru_reset_fwd(ssm_view gates_x, ssm_view gates_h, ssm_view h_prev, ssm_view rh_f32, ssm_hview rh_hl8, int B,
                          int Hc, int H, int W, int flags, void *stream);
int ssm_convgru_update_fwd(ssm_view gates_x, ssm_view gates_h, ssm_view cand_x, ssm_view cand_h, ssm_view h_prev,
                           ssm_view h_f32, ssm_hview h_hl8, int B, int Hc, int H, int W, int flags, void *stream);

/* Adjoints of the cells above (training through the recurrent bottleneck; the gate convolutions' own gradients are the conv
 * backward entry points).  fp32 views.
 *  ssm_convlstm_cell_bwd   d h', d c' (NULL = 0) -> dgates [4*Hc] and d c          (gates_h / c_prev NULL at the first step)
 *  ssm_convgru_reset_bwd   d(rh) -> dgates[0:Hc] (gamma) and d h;  the caller zeroes / owns dgates[Hc:2Hc]
 *  ssm_convgru_update_bwd  d h' -> dgates[Hc:2Hc] (beta), d cand and d h (h_prev / dh_prev NULL at the first step);
 *                          `gates` = the summed pre-activations [gamma|beta], `cand` = the candidate pre-activation          */
int ssm_convlstm_cell_bwd(ssm_view gates_x, ssm_view gates_h, ssm_view c_prev, ssm_view dh, ssm_view dc_next, ssm_view dgates,
                          ssm_view dc_prev, int B, int Hc, int H, int W, void *stream);
int ssm_convgru_reset_bwd(ssm_view gates, ssm_view h_prev, ssm_view drh, ssm_view dgates, ssm_view dh_prev, int B, int Hc, int H, int W,
                          void *stream);
int ssm_convgru_update_bwd(ssm_view gates, ssm_view cand, ssm_view h_prev, ssm_view dh_next, ssm_view dgates, ssm_view dcand,
                           ssm_view dh_prev, int B, int Hc, int H, int W, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SSM_HIP_H */
