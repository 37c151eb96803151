"""Streamed slow-motion video: YUV4MPEG2 in, YUV4MPEG2 out, colour conversion on the GPU.

  Y4MReader / Y4MWriter   the one video container that needs no codec (every player and ffmpeg read and write it, pipes included):
                          a text header `YUV4MPEG2 W H F I A C X...`, then `FRAME` records of planar Y, U, V: 8-bit 4:2:0 and 4:4:4, and
                          with extended=True also 4:2:2 and 9 to 16 bits per sample (C422, C420p10, C422p10, C444p12, ...: EXTENDED_TAGS)
  yuv_table               the conversion constants of a bit depth, float64 rounded once to fp32: what csrc/ssm_video.hip and the
                          yardsticks both read; `bits` (the significant bits of a sample, 8 to 16) lives in this table alone
  table_index             BT.2020 (MATRICES["bt2020"]) has a table of its own, yuv_table(bits, BT2020): the index of a matrix's rows in its table
  yuv_to_frames_host /    numpy float32 yardsticks that spell the two kernels' operations in the kernels' order: the fixed points the
  frames_to_yuv_host      kernels are held to bit for bit (as scripts/utils/flo_utils.py is for csrc/ssm_flow.hip)
  frames_from_yuv /       the kernels: payloads on the device <-> the path's normalised, padded fp32 planes, in the visualiser's
  frames_to_yuv           convention (scripts/visualize_interpolation.py:61-88,223-268)
  VideoInterpolator       the streamed loop: every leg of a pass (H2D, ingest, the pair pipeline, egress, D2H) is queued on the pass's HIP
                          stream, a writer thread drains a ring of pinned buffers in order; memory does not depend on the clip's length
  PassRing / read_passes  what its four modes (fixed grid, timeline, shutter, fields) share beside the prologue, the Clip with its two conversions and
  / read_blocks /         their buffers: the ring with its writer thread and failure protocol (no GPU in it), the planners' read loop and the
  upload_times            block modes' (pairs_per_batch new units behind a carried one: fixed grid, fields, video_score's scorer), a pass's times
  PairOptions             the per-pair options of the fixed grid and the timeline in one per-run object: scene cuts, static blocks, the window
                          of a letterboxed clip - their buffers, the carry of row 0 (two protocols, argued there), their calls, the writer's rows

  Timeline / PassPlanner  any output rate and speed: where each output frame sits on the input's clock, exactly (Fractions, closed form),
                          and the bookkeeping of the passes that follow it - VideoInterpolator(target_rate=, speed=)
  accumulate_host /       the shutter: an output frame as the mean of `samples` sub-frames over the open part of its interval
  ShutterPlanner          (Timeline(step, shutter=, samples=)), summed on the GPU in time order by ssm_frames_accumulate_fwd, whose numpy
                          yardstick accumulate_host is; the bookkeeping of its passes - VideoInterpolator(shutter=, shutter_samples=)
  light_curve /           the shutter in linear light: the same kernel's second mode (ssm_frames_accumulate_light_fwd, held to an error bound
  accumulate_light_host   against this float64 yardstick), the sub-frames decoded to light by one of LIGHT_CURVES before they are summed, the
                          mean encoded again - VideoInterpolator(shutter_light=); "coded", the default, is the mean of the coded values
  hdr_light               the shutter in the light of HDR clips, "pq" and "hlg" (HDR_LIGHTS): the kind and row ssm_frames_accumulate_hdr_fwd takes
  hdr_decode_host / hdr_encode_host   the BT.2100 PQ EOTF and inverse HLG OETF and their inverses, in float64 or in the kernel's fp32 steps
  accumulate_hdr_host     the float64 yardstick of ssm_frames_accumulate_hdr_fwd, accumulate_light_host with those in place of a curve's row
  shutter_window /        the weights of a shutter's sub-frames: "box" (all alike: the calls above, untouched), "triangle", "hann", "gauss[:K]",
  parse_shutter_window    sample j at (j + 1/2) / S of the open interval, and the scale 1 / sum that closes an output; the three yardsticks take
                          weights= and are then those of the ssm_frames_accumulate*_weighted_fwd siblings (coded: bit for bit; light and HDR:
                          bounds of tests/test_video_window_cpu.py) - VideoInterpolator(shutter_window=)
  luma_sad_host / luma_sad   scene cuts: per frame pair the exact sum of |difference| of the 8-bit Y planes, by numpy (the yardstick) and by
  / SceneCuts             ssm_luma_sad_fwd on the payloads as they stand on the device; the decision from those sums in Fractions, with no
                          GPU in it - VideoInterpolator(scene_cut=): at a cut the output repeats the nearer input frame instead of a morph
  split_fields_host /     interlaced clips: a frame's two fields (the even and the odd rows of every plane) as payloads of their own, and frames
  weave_fields_host       woven from kept fields and synthesised ones or integer line averages - the numpy definitions ssm_fields_split_fwd
  / field_outputs         and ssm_fields_weave_fwd (fields_split, fields_weave) are held to bit for bit; which field is which time under
                          tff / bff and which pairs run - VideoInterpolator(deinterlace=): 2n progressive frames of an n-frame clip (_run_fields)
  LookAheadSource         what the four readers in front of the loop share (FieldOrderSource, TelecineSource, RepeatSource, ActiveSource): the
                          mirrored format attributes, the chunk's pinned and device buffers made once, the measuring step of a chunk on a
                          stream of its own (one H2D, one kernel entry, one D2H per result, one event wait), the read loop with its carried
                          frames, probe and replay, and the one hand-out path; a source adds its kernel, its carry, its decider, its frames
  field_order_sums_host / interlaced clips, the field order from the data: per frame the comb sums A0, A1, D of its luma plane against the frame
  field_order_sums /      before and the frame after, by numpy and by ssm_field_order_sums_fwd; the kind of a frame (field_kind) and the verdict
  FieldVerdict /          of a probe in Python ints; the reader that probes and replays in front of the loop - VideoInterpolator(field_probe=):
  FieldOrderSource        the order of a deinterlace="auto" run whose header says Ip or I?, a warning or a report everywhere else
  telecine_host /         film in 3:2 pulldown: the pulldown and its removal in numpy, the per-field luma differences by numpy and by
  detelecine_host /       ssm_field_diff_fwd, the cadence decision from those sums in Python ints (Cadence), and the reader that undoes the
  field_diff / Cadence    pulldown in front of the loop - TelecineSource(reader, dev): downstream sees the film's frames as a progressive clip at
  / TelecineSource        detelecine_rate; every mode of VideoInterpolator is unchanged by it
  block_sad_host /        repeated frames (animation on twos and threes, 24 -> 60 by repetition, filled drops): per pair and plane the largest
  block_sad / Repeats /   8 x 8 block sum of |difference| and the number of blocks above `lo`, by numpy and by ssm_block_sad_fwd; the repeat
  dedup_host /            decision and the runs in Python ints and Fractions; the reader that takes the repaired repeats out in front of the
  RepeatSource /          loop and the timeline over the frames that stay, which puts synthesised frames where the repeats stood -
  GapTimeline             VideoInterpolator(dedup=, dedup_max=): the fixed grid's frame count and rate, every other mode unchanged
  active_counts_host /    letterboxed clips: per frame the luma samples above a limit of every row and column, by numpy and by
  luma_counts / ActiveArea ssm_luma_counts_fwd; the rectangle that holds every active line of the probed frames, in Python ints and Fractions;
  / cut_window_host /     a rectangle of a payload as a payload of its own and back (ssm_window_cut_fwd, window_cut, is held to the cut byte
  paste_window_host /     for byte); the reader that probes, decides and watches in front of the loop - VideoInterpolator(active=,
  ActiveSource            active_probe=): the run is the cropped clip's, the bars of a synthesised frame are the nearer input frame's bytes
  static_paste_host /     blocks that do not change (a logo, subtitles, a timecode, a locked-off background): where the two frames of a pair agree
  static_paste /          on an 8 x 8 block - luma and the chroma under it, sum of |difference| at most `lo` - every frame between them carries the
  parse_static            left frame's samples of that block, by numpy and by ssm_static_paste_fwd on the pass's stream; the number of such
                          blocks per pair - VideoInterpolator(static=): the fixed grid and the timeline, every other mode unchanged
  flow_paste_host /       the flow check's per-block fallback: where more than K of an 8 x 8 block's 64 luma pixels are inconsistent in at least
  flow_paste /            one direction of a pair's mask (flow_eval.flow_consistency), every frame between the pair carries the NEARER frame's
  parse_flow_blocks       samples of that block, by numpy and by ssm_flow_paste_fwd on the pass's stream; the number of such blocks per pair -
                          VideoInterpolator(flow_check=, flow_blocks=): the fixed grid and the timeline, every other mode unchanged
  flow_mix_host /         the same blocks carrying the cross-fade a (1 - t) + b t of the pair's two frames at the output's exact time, rounded
  flow_mix /              half up, by numpy and by ssm_flow_mix_fwd; fixed_mix, times_mix and flow_mix_den name a pair's times as three
  parse_flow_fallback     launch scalars - VideoInterpolator(flow_blocks=, flow_fallback="mix"); "nearer" is the run without it
  (ssm_amd/video_score.py) hold-out scoring: the clip against its own held-out frames, plane_sse / HoldOutScorer on this loop's ring, Clip and
                          buffers; the PSNR of what VideoInterpolator(upsample_rate=hold) would write - this module is unchanged by it

Formats.  A sample of more than 8 bits is a 16-bit little-endian word with the value in its low bits (ffmpeg's convention); payloads stay
[N, frame_bytes] uint8 whatever the depth, so the ring, the pinned slots and "input frames reach the output as their own bytes" do not
depend on it.  4:2:2 chroma is co-sited with the even luma columns, as the Y4M specification states; C420pB carries no siting and is
read as C420 is, centred.  The fp32 pipeline between ingest and egress is the same for every format: the output has the input's format.

Out of scope: codecs, audio, output in another format than the input (8-bit in, 10-bit out), mono, 4:1:1 and alpha planes, a siting
override for C420pB, big-endian samples, scene cuts above 8 bits (ssm_luma_sad_fwd and the score's / 255 are 8-bit), the recurrent
configuration (N_FRAMES > 2); asymmetric or user-supplied shutter weights, shutter windows on the fixed grid
(upsample_rate, slowmo), any statement about which window looks best, a light curve chosen from the clip's tags, an OOTF for the HDR lights (PQ display light and HLG scene light are taken as they are), BT.2020 constant luminance, a shutter centred on the frame's instant or open for longer than the frame interval,
variable-rate input, speeds that change within a clip; a default scene-cut threshold, fades and dissolves, cuts judged on chroma,
skipping the GPU work of a cut pair, scene cuts together with a shutter; a measure of quality other than video_score's PSNR against
held-out frames (SSIM, VMAF), and that score for the timeline, shutter and scene-cut outputs; of interlaced clips: mixed field order (Im),
scene cuts between fields, deinterlacing and retiming in one pass (chain two runs), the true vertical
chroma siting of a 4:2:0 field (a quarter line off the layout's rule, which is what the fields are converted with); of pulldown removal:
2:2, 2:3:3:2 and mixed cadences, soft telecine, the orphan field at an edit inside a cycle, comb metrics, noisy or compressed sources;
of repeated frames: timestamps (timecode files), dropping repeats instead of repairing them, dedup together with target_rate, speed,
shutter, scene_cut or deinterlace (chain two runs), a scene cut on the frame after a run, comparison against a run's first frame,
agreement with ffmpeg's mpdecimate frame for frame, noisy or compressed footage; of letterboxed clips: a rectangle that changes inside a
clip, coloured bars, re-planning when a later frame exceeds the rectangle, active together with shutter, deinterlace or dedup (chain two
runs), noisy or compressed bars; of the field probe: watching frames behind the probe, Im, a per-frame order, detection on chroma, noisy
or compressed footage (every clip it was tried on is synthetic), agreement with ffmpeg's idet frame for frame; of static blocks: smoothing the
seams between kept and synthesised blocks, growing or eroding the static set, per-pixel masks, a default lo, noisy or compressed footage
(where no block agrees exactly), static together with shutter, deinterlace, dedup, active or a recurrent model (chain two runs), skipping
the network on frames that are static throughout.
"""
import ctypes
import functools
import queue
import re
import sys
import threading
from collections import namedtuple
from fractions import Fraction

import numpy as np
import torch

from . import hipbind as hb
from .frames import _f3, cfg_mean_std, padded_dims

BT601, BT709, BT2020 = 0, 1, 2          # BT2020: non-constant luminance; a name of this module, not an index the entry points take
LIMITED, FULL = 0, 1
CENTRED, COSITED, C444, C422 = 0, 1, 2, 3          # chroma siting / plane layout (include/ssm_hip.h SSM_YUV_*)
YUV_ROW = 20
MATRICES = {"bt601": BT601, "bt709": BT709, "bt2020": BT2020}
RANGES = {"limited": LIMITED, "full": FULL}
# Y4M colour-space tags: accepted -> siting; refused ones are named in the error
CHROMA_TAGS = {"420": CENTRED, "420jpeg": CENTRED, "420mpeg2": COSITED, "444": C444}
# with extended=True: tag -> (layout, bits); samples of more than 8 bits are 16-bit little-endian words
DEEP_BITS = (9, 10, 12, 14, 16)
EXTENDED_TAGS = {tag: (lay, 8) for tag, lay in CHROMA_TAGS.items()}
EXTENDED_TAGS["422"] = (C422, 8)
for _b in DEEP_BITS:
    EXTENDED_TAGS.update({"420p%d" % _b: (CENTRED, _b), "422p%d" % _b: (C422, _b), "444p%d" % _b: (C444, _b)})
_TAGS_8BIT = "8-bit C420, C420jpeg, C420mpeg2 and C444 are"
_TAGS_EXTENDED = "C420, C420jpeg, C420mpeg2, C422, C444 and C420pB, C422pB, C444pB with B in 9, 10, 12, 14, 16 are"


def chroma_format(tag, extended=False):
    """(layout, bits) of a Y4M colour-space tag; a tag outside the set - the 8-bit one, or with `extended` EXTENDED_TAGS - is refused by name."""
    if extended:
        if tag not in EXTENDED_TAGS:
            raise Y4MError("Y4M colour space C%s is not supported (%s)" % (tag, _TAGS_EXTENDED))
        return EXTENDED_TAGS[tag]
    if tag not in CHROMA_TAGS:
        raise Y4MError("Y4M colour space C%s is not supported (%s)" % (tag, _TAGS_8BIT))
    return CHROMA_TAGS[tag], 8


def sample_bytes(bits):
    """Bytes of a sample of `bits` significant bits (8 to 16): 1, or 2 above 8."""
    if isinstance(bits, bool) or int(bits) != bits or not 8 <= bits <= 16:
        raise ValueError("bits = %r: a sample has 8 to 16 significant bits" % (bits,))
    return 1 if bits == 8 else 2
_KRKB = {BT601: (0.299, 0.114), BT709: (0.2126, 0.0722)}          # the rows of the table every entry point has always been given
_KRKB_OWN = {BT2020: (0.2627, 0.0593)}                            # matrices with a table of their own: one matrix, its rows at index 0


# Light curves (include/ssm_hip.h): name -> (thr, slope, a, g) of  decode(c) = c <= thr ? c / slope : ((c + a) / (1 + a)) ^ g  and
# encode(L) = L <= thr / slope ? L * slope : (1 + a) * L ^ (1 / g) - a.  bt709 is the inverse of the BT.709 camera curve V = 4.5 L below
# beta, alpha L^0.45 - (alpha - 1) from there on.  The standard prints beta = 0.018 and alpha = 1.099; with those three digits the two
# pieces miss each other at the join by 5.5e-5 of L (2.5e-4 of c).  alpha and beta below are the solution of the two conditions those
# digits were rounded from - the pieces meet in value and in slope: 4.5 beta = alpha beta^0.45 - (alpha - 1), 4.5 = 0.45 alpha beta^-0.55
# (BT.2020 prints the same numbers as 1.0993 and 0.0181) - so thr = 4.5 beta = 0.08124..., a = alpha - 1 = 0.09930....
_BT709_ALPHA, _BT709_BETA = 1.09929682680944, 0.018053968510807
LIGHT_CURVES = {"bt709": (4.5 * _BT709_BETA, 4.5, _BT709_ALPHA - 1.0, 1.0 / 0.45),
                "srgb": (0.04045, 12.92, 0.055, 2.4),
                "bt1886": (0.0, 1.0, 0.0, 2.4)}
LIGHT_ROW = hb.SSM_LIGHT_ROW
SHUTTER_LIGHTS = ("coded",) + tuple(LIGHT_CURVES)          # "coded": the mean of the coded values, no curve


def light_curve(name):
    """The row of LIGHT_ROW float32 constants of a light curve, every one evaluated in float64 and rounded once (layout: include/ssm_hip.h):
    thr, 1/slope, a, 1/(1+a), g, thr/slope, slope, 1+a, 1/g.  What ssm_frames_accumulate_light_fwd and accumulate_light_host both read."""
    if name not in LIGHT_CURVES:
        raise ValueError("unknown light curve %r: the curves are %s" % (name, ", ".join(LIGHT_CURVES)))
    thr, slope, a, g = LIGHT_CURVES[name]
    return np.array([thr, 1.0 / slope, a, 1.0 / (1.0 + a), g, thr / slope, slope, 1.0 + a, 1.0 / g], dtype=np.float64).astype(np.float32)


# HDR transfer functions as the shutter's light (include/ssm_hip.h): BT.2100 PQ - display light as a fraction of 10000 cd/m2 - and HLG -
# scene light - neither with an OOTF.  They are no power laws with a linear toe, so they have a table, a row layout and an entry point of
# their own (ssm_frames_accumulate_hdr_fwd); LIGHT_CURVES and SHUTTER_LIGHTS stay what they were.  The PQ constants are dyadic fractions,
# exact in fp32; HLG's b and cc are evaluated in float64 from a, not taken from their printed digits.
PQ_M1, PQ_M2 = 2610.0 / 16384.0, 2523.0 / 4096.0 * 128.0
PQ_C1, PQ_C2, PQ_C3 = 3424.0 / 4096.0, 2413.0 / 4096.0 * 32.0, 2392.0 / 4096.0 * 32.0
HLG_A = 0.17883277
HLG_B = 1.0 - 4.0 * HLG_A
HLG_CC = 0.5 - HLG_A * float(np.log(4.0 * HLG_A))
HDR_ROW = hb.SSM_HDR_ROW
HDR_KINDS = {"pq": hb.SSM_HDR_PQ, "hlg": hb.SSM_HDR_HLG}
HDR_LIGHTS = tuple(HDR_KINDS)


def hdr_light(name):
    """(kind, row) of an HDR light: the kind ssm_frames_accumulate_hdr_fwd takes and its HDR_ROW float32 constants, every one evaluated in
    float64 and rounded once (layout: include/ssm_hip.h).  pq: 1/m2, c1, c2, c3, 1/m1, m1, m2, 0.  hlg: 1/3, log2(e)/a, cc, b, 1/12,
    a ln 2, 0, 0."""
    if name not in HDR_KINDS:
        raise ValueError("unknown HDR light %r: the HDR lights are %s" % (name, ", ".join(HDR_LIGHTS)))
    if name == "pq":
        row = [1.0 / PQ_M2, PQ_C1, PQ_C2, PQ_C3, 1.0 / PQ_M1, PQ_M1, PQ_M2, 0.0]
    else:
        row = [1.0 / 3.0, float(np.log2(np.e)) / HLG_A, HLG_CC, HLG_B, 1.0 / 12.0, HLG_A * float(np.log(2.0)), 0.0, 0.0]
    return HDR_KINDS[name], np.array(row, dtype=np.float64).astype(np.float32)


def parse_shutter_light(name):
    """"coded", the name of a light curve or of an HDR light, as given; anything else is refused by name."""
    if name not in SHUTTER_LIGHTS + HDR_LIGHTS:
        raise ValueError("unknown shutter_light %r: it is one of %s" % (name, ", ".join(SHUTTER_LIGHTS + HDR_LIGHTS)))
    return name


def table_index(matrix):
    """The index at which a matrix's rows sit in its table: what the entry points take as `matrix` (they refuse anything but 0 and 1).
    BT601 and BT709 share yuv_table(bits) at their own numbers; BT2020 has yuv_table(bits, BT2020) to itself, at 0."""
    if matrix in _KRKB:
        return matrix
    if matrix in _KRKB_OWN:
        return 0
    raise ValueError("unknown matrix %r: the matrices are %s" % (matrix, ", ".join(MATRICES)))


def yuv_table(bits=8, matrix=None):
    """[2 matrices][2 ranges][YUV_ROW] float32 for samples of `bits` significant bits: every constant evaluated in float64 and rounded
    once (layout: include/ssm_hip.h).  With s = 2^(bits-8) and peak = 2^bits - 1 the codes map to the 0 .. 255 units the kernels work in:
    limited 16 s .. 235 s (240 s), full 0 .. peak.  bits = 8 gives s = 1 and peak = 255: the 8-bit table, bit for bit.
    matrix = None, BT601 or BT709: that table, the one of BT.601 and BT.709.  matrix = BT2020: [1][2 ranges][YUV_ROW], the table of
    BT.2020 alone, the same expressions on its Kr and Kb; table_index says where a matrix's rows sit."""
    sample_bytes(bits)
    s, peak = float(1 << (bits - 8)), float((1 << bits) - 1)
    own = matrix is not None and matrix not in _KRKB
    table_index(BT601 if matrix is None else matrix)
    t = np.zeros((1 if own else 2, 2, YUV_ROW), dtype=np.float64)
    for m, (kr, kb) in ({0: _KRKB_OWN[matrix]} if own else _KRKB).items():
        kg = 1.0 - kr - kb
        for r in (LIMITED, FULL):
            lim = r == LIMITED
            t[m, r, :19] = [kr, kg, kb,
                            2.0 * (1.0 - kr), 2.0 * (1.0 - kb) * kb / kg, 2.0 * (1.0 - kr) * kr / kg, 2.0 * (1.0 - kb),
                            1.0 / (2.0 * (1.0 - kb)), 1.0 / (2.0 * (1.0 - kr)),
                            255.0 / (219.0 * s) if lim else 255.0 / peak, 255.0 / (224.0 * s) if lim else 255.0 / peak,
                            219.0 * s / 255.0 if lim else peak / 255.0, 224.0 * s / 255.0 if lim else peak / 255.0,
                            16.0 * s if lim else 0.0, 128.0 * s,
                            16.0 * s if lim else 0.0, 235.0 * s if lim else peak, 16.0 * s if lim else 0.0, 240.0 * s if lim else peak]
    return t.astype(np.float32)


_table_c = {}


def _table_ptr(bits=8, matrix=None):
    """The table of a bit depth (and of the matrix, where it has one of its own) as the C array the entry points take; one each, kept."""
    key = bits if matrix is None or matrix in _KRKB else (bits, matrix)
    if key not in _table_c:
        flat = yuv_table(bits, matrix).reshape(-1)
        _table_c[key] = (ctypes.c_float * flat.size)(*[float(v) for v in flat])
    return _table_c[key]


def chroma_dims(h, w, siting, bits=8):
    if siting == C444:
        return h, w
    return (h, (w + 1) // 2) if siting == C422 else ((h + 1) // 2, (w + 1) // 2)


def frame_bytes(h, w, siting, bits=8):
    ch, cw = chroma_dims(h, w, siting)
    return (h * w + 2 * ch * cw) * sample_bytes(bits)


def split_planes(payload, h, w, siting, bits=8):
    """[N, frame_bytes] uint8 -> Y [N,h,w], U, V [N,ch,cw] (views); with bits > 8 the payload is a numpy array and the planes are its
    little-endian uint16 words."""
    ch, cw = chroma_dims(h, w, siting)
    if sample_bytes(bits) == 2:
        payload = payload.view("<u2")
    n = payload.shape[0]
    y = payload[:, :h * w].reshape(n, h, w)
    u = payload[:, h * w:h * w + ch * cw].reshape(n, ch, cw)
    v = payload[:, h * w + ch * cw:].reshape(n, ch, cw)
    return y, u, v


def default_matrix(h):
    """BT.709 for HD (720 rows and up), BT.601 below: what players assume of untagged material."""
    return BT709 if h >= 720 else BT601


# ---- numpy float32 yardsticks: the kernels' operations in the kernels' order -------------------------------------------------------
_F = np.float32


def _upsample_host(c, h, w, siting):
    """Chroma plane [N,ch,cw] float32 -> [N,h,w]: bilinear, indices clamped; columns first, then rows, as the kernel.  4:2:2: columns only."""
    ch, cw = c.shape[1:]
    x = np.arange(w)
    j, odd = x // 2, (x % 2) == 1
    a0, a1, b1, b2 = (_F(0.0), _F(1.0), _F(0.5), _F(0.5)) if siting in (COSITED, C422) else (_F(0.25), _F(0.75), _F(0.75), _F(0.25))
    ia = np.clip(np.where(odd, j, j - 1), 0, cw - 1)
    ib = np.clip(np.where(odd, j + 1, j), 0, cw - 1)
    wa = np.where(odd, b1, a0).astype(_F)
    wb = np.where(odd, b2, a1).astype(_F)
    hz = wa * c[:, :, ia] + wb * c[:, :, ib]
    if siting == C422:
        return hz
    y = np.arange(h)
    i, odd = y // 2, (y % 2) == 1
    ia = np.clip(np.where(odd, i, i - 1), 0, ch - 1)
    ib = np.clip(np.where(odd, i + 1, i), 0, ch - 1)
    wa = np.where(odd, _F(0.75), _F(0.25)).astype(_F)[None, :, None]
    wb = np.where(odd, _F(0.25), _F(0.75)).astype(_F)[None, :, None]
    return wa * hz[:, ia] + wb * hz[:, ib]


def yuv_to_frames_host(payload, h, w, siting=CENTRED, matrix=BT709, color_range=LIMITED, mean=None, std=None, pad_before_norm=True, *,
                       bits=8):
    """Yardstick of ssm_frames_from_yuv_fwd / ssm_frames_from_yuvx_fwd: [N, frame_bytes] uint8 (numpy) -> [N,3,Hp,Wp] float32."""
    if mean is None:
        mean, std = cfg_mean_std(None)
    k = yuv_table(bits, matrix)[table_index(matrix), color_range]
    kr, kg, kb, rv, gu, gv, bu, cbs, crs, ys, cs, iys, ics, yoff, coff = k[:15]
    payload = np.ascontiguousarray(payload).reshape(-1, frame_bytes(h, w, siting, bits))
    yq, uq, vq = split_planes(payload, h, w, siting, bits)
    yl, cu, cv = yq.astype(_F), uq.astype(_F), vq.astype(_F)
    if siting != C444:
        cu, cv = _upsample_host(cu, h, w, siting), _upsample_host(cv, h, w, siting)
    yl = (yl - yoff) * ys
    cb = (cu - coff) * cs
    cr = (cv - coff) * cs
    rgb = (yl + rv * cr, (yl - gu * cb) - gv * cr, yl + bu * cb)
    (hp, wp), (top, left) = padded_dims(h, w)
    out = np.zeros((payload.shape[0], 3, hp, wp), dtype=_F)
    for p in range(3):
        m, s = _F(mean[p]), _F(std[p])
        if pad_before_norm:
            out[:, p] = (_F(0.0) / _F(255.0) - m) / s
        out[:, p, top:top + h, left:left + w] = (np.clip(rgb[p], _F(0.0), _F(255.0)) / _F(255.0) - m) / s
    return out


def frames_to_yuv_host(x, h, w, siting=CENTRED, matrix=BT709, color_range=LIMITED, mean=None, std=None, *, bits=8):
    """Yardstick of ssm_frames_to_yuv_fwd / ssm_frames_to_yuvx_fwd: [N,3,Hp,Wp] float32 (numpy, finite) -> [N, frame_bytes] uint8."""
    if mean is None:
        mean, std = cfg_mean_std(None)
    k = yuv_table(bits, matrix)[table_index(matrix), color_range]
    kr, kg, kb, rv, gu, gv, bu, cbs, crs, ys, cs, iys, ics, yoff, coff, ylo, yhi, clo, chi = k[:19]
    x = np.asarray(x, dtype=_F)
    n, _, hp, wp = x.shape
    top, left = (hp - h) // 2, (wp - w) // 2
    rgb = []
    for p in range(3):
        v = x[:, p, top:top + h, left:left + w] * _F(std[p]) + _F(mean[p])
        rgb.append(v * _F(255.0))
    r, g, b = rgb
    yf = (kr * r + kg * g) + kb * b
    cb = (b - yf) * cbs
    cr = (r - yf) * crs

    def sub(c):
        if siting == C444:
            return c
        ch, cw = chroma_dims(h, w, siting)
        cx, cy = np.arange(cw), np.arange(ch)
        c0, c1 = 2 * cx, np.minimum(2 * cx + 1, w - 1)
        r0, r1 = 2 * cy, np.minimum(2 * cy + 1, h - 1)
        if siting in (COSITED, C422):
            cl = np.maximum(2 * cx - 1, 0)
            hz = ((c[:, :, cl] + _F(2.0) * c[:, :, c0]) + c[:, :, c1]) * _F(0.25)
            return hz if siting == C422 else (hz[:, r0] + hz[:, r1]) * _F(0.5)
        t, bt = c[:, r0], c[:, r1]
        return ((t[:, :, c0] + t[:, :, c1]) + (bt[:, :, c0] + bt[:, :, c1])) * _F(0.25)

    def code(v, scale, off, lo, hi):
        return np.clip(np.rint(v * scale + off), lo, hi).astype(np.uint8 if bits == 8 else "<u2")

    planes = [code(yf, iys, yoff, ylo, yhi), code(sub(cb), ics, coff, clo, chi), code(sub(cr), ics, coff, clo, chi)]
    return np.concatenate([p.reshape(n, -1) for p in planes], axis=1).view(np.uint8)


def _call_weights(weights, n, dt):
    """A weighted call's N weights as `dt` values of the fp32 weights the kernel is given."""
    w = np.asarray(weights, dtype=_F)
    assert w.shape == (n,) and np.all(np.isfinite(w)), "a weighted call takes one finite weight per frame (%d frames, weights %r)" % (n, weights)
    return w.astype(dt)


def accumulate_host(frames, acc, init, scale, weights=None):
    """Yardstick of ssm_frames_accumulate_fwd: frames [N,C,H,W] float32 (numpy) summed into acc [1,C,H,W] or [C,H,W] float32, in place:
    s = frames[0] if init else acc + frames[0]; s = s + frames[n] for n = 1 .. N-1; acc = s * scale - every step rounded to float32.
    weights (N floats): the yardstick of ssm_frames_accumulate_weighted_fwd, p_n = weights[n] * frames[n] in place of frames[n], the
    product one more rounded float32 operation; None is the arithmetic above, line for line."""
    frames = np.asarray(frames, dtype=_F)
    assert acc.dtype == _F and frames.ndim == 4 and frames.shape[0] >= 1 and init in (0, 1, False, True)
    dst = acc[0] if acc.ndim == 4 else acc
    assert dst.shape == frames.shape[1:] and (acc.ndim == 3 or acc.shape[0] == 1)
    if weights is None:
        s = frames[0].copy() if init else dst + frames[0]
        for n in range(1, frames.shape[0]):
            s = s + frames[n]
    else:
        w = _call_weights(weights, frames.shape[0], _F)
        s = w[0] * frames[0] if init else dst + w[0] * frames[0]
        for n in range(1, frames.shape[0]):
            s = s + w[n] * frames[n]
    dst[...] = s * _F(scale)
    return acc


def _light_constants(curve, dt):
    """(thr, 1/slope, a, 1/(1+a), g, thr/slope, slope, 1+a, 1/g) in `dt`.  float32: the row as it is, what the kernel multiplies by.
    float64: the row's thr, slope, a and g - fp32 values - with the other five taken from them in float64, so that encode inverts decode to
    float64's own precision instead of the 1e-7 by which two rounded reciprocals miss each other; the kernel's distance from that is part
    of its bound (tests/test_video_light_cpu.py)."""
    row = np.asarray(curve, np.float32)
    assert row.shape == (LIGHT_ROW,), "a light curve's row holds %d floats" % LIGHT_ROW
    if dt is np.float32:
        return tuple(row)
    thr, a, g, slope = (np.float64(row[i]) for i in (0, 2, 4, 6))
    return thr, 1.0 / slope, a, 1.0 / (1.0 + a), g, thr / slope, slope, 1.0 + a, 1.0 / g


def light_decode_host(c, curve, dtype=np.float64):
    """decode(c) of a light curve's row, element-wise in `dtype`: c <= thr ? c * (1/slope) : ((c + a) * (1/(1+a))) ^ g."""
    dt = np.dtype(dtype).type
    thr, islope, a, i1a, g = _light_constants(curve, dt)[:5]
    c = np.asarray(c, dtype=dt)
    return np.where(c <= thr, c * islope, np.power(np.maximum((c + a) * i1a, dt(0.0)), g))


def light_encode_host(lum, curve, dtype=np.float64):
    """encode(L) of a light curve's row, element-wise in `dtype`: L <= thr/slope ? L * slope : (1+a) * L ^ (1/g) - a."""
    dt = np.dtype(dtype).type
    k = _light_constants(curve, dt)
    a, (lthr, slope, a1, ig) = k[2], k[5:9]
    lum = np.asarray(lum, dtype=dt)
    return np.where(lum <= lthr, lum * slope, a1 * np.power(np.maximum(lum, dt(0.0)), ig) - a)


def accumulate_light_host(frames, acc, init, scale, mean, std, curve, encode, dtype=np.float64, weights=None):
    """Yardstick of ssm_frames_accumulate_light_fwd: frames [N,3,H,W] float32 (numpy, finite) summed as light into acc [1,3,H,W] or
    [3,H,W] of `dtype`, in place, the kernel's operations in the kernel's order, every one in `dtype`:
      dec(v) = 0 if v <= black[p] else decode(clip(v * std[p] + mean[p], 0, 1)), black = (0 / 255 - mean) / std in fp32 as the ingest has it;
      s = dec(frames[0]) if init else acc + dec(frames[0]);  s = s + dec(frames[n]), n = 1 .. N-1;  r = s * scale;
      acc = (encode(r) - mean[p]) / std[p] if encode else r.
    mean and std enter as the fp32 values the kernel is given, the curve's row as _light_constants says; scale is taken as it is (the
    kernel takes an fp32 one: give np.float32(1 / S) to compare).  dtype = float64: the fixed point the kernel is held to within the
    bound of tests/test_video_light_cpu.py (x ^ e is numpy's power).  dtype = float32: what plain fp32 arithmetic gives; it is not the
    kernel bit for bit, whose power is 2 ^ (e log2 x) by the hardware's instructions.
    weights (N floats): the yardstick of ssm_frames_accumulate_light_weighted_fwd, weights[n] * dec(frames[n]) in place of dec(frames[n]),
    the fp32 weights taken to `dtype` as they are (bounds: tests/test_video_window_cpu.py); None is the arithmetic above, line for line."""
    dt = np.dtype(dtype).type
    assert dt in (np.float32, np.float64), "dtype is numpy's float32 or float64"
    frames = np.asarray(frames, dtype=_F)
    assert acc.dtype == dt and frames.ndim == 4 and frames.shape[0] >= 1 and frames.shape[1] == 3 and init in (0, 1, False, True) and \
        encode in (0, 1, False, True)
    dst = acc[0] if acc.ndim == 4 else acc
    assert dst.shape == frames.shape[1:] and (acc.ndim == 3 or acc.shape[0] == 1)
    m32, s32 = np.asarray(mean, dtype=_F).reshape(3, 1, 1), np.asarray(std, dtype=_F).reshape(3, 1, 1)
    black = (_F(0.0) / _F(255.0) - m32) / s32
    m, sd = m32.astype(dt), s32.astype(dt)

    def dec(v):
        c = np.where(v <= black, dt(0.0), np.clip(v.astype(dt) * sd + m, dt(0.0), dt(1.0)))
        return light_decode_host(c, curve, dt)

    if weights is None:
        s = dec(frames[0]) if init else dst + dec(frames[0])
        for n in range(1, frames.shape[0]):
            s = s + dec(frames[n])
    else:
        w = _call_weights(weights, frames.shape[0], dt)
        s = w[0] * dec(frames[0]) if init else dst + w[0] * dec(frames[0])
        for n in range(1, frames.shape[0]):
            s = s + w[n] * dec(frames[n])
    r = s * dt(scale)
    dst[...] = (light_encode_host(r, curve, dt) - m) / sd if encode else r
    return acc


def _pow_host(x, e, dt):
    """x ^ e for x >= 0 in `dt`.  float64: numpy's power.  float32: 2 ^ (e log2 x) in three rounded steps, as the kernel's pow_fast
    (numpy's log2 and exp2 in place of the hardware's instructions); x = 0 gives 2 ^ -inf = 0."""
    if dt is np.float64:
        return np.power(x, e)
    with np.errstate(divide="ignore"):
        return np.exp2(dt(e) * np.log2(x))


def hdr_decode_host(c, name, dtype=np.float64):
    """decode(c) of an HDR light (include/ssm_hip.h), element-wise in `dtype`, c in [0, 1].  float64: the defining formulas on the float64
    constants.  float32: the kernel's steps on hdr_light(name)'s row, one rounded operation each."""
    dt = np.dtype(dtype).type
    c = np.asarray(c, dtype=dt)
    if dt is np.float64:
        if name == "pq":
            p = np.power(c, 1.0 / PQ_M2)
            return np.power(np.maximum(p - PQ_C1, 0.0) / (PQ_C2 - PQ_C3 * p), 1.0 / PQ_M1)
        return np.where(c <= 0.5, c * c / 3.0, (np.exp((c - HLG_CC) / HLG_A) + HLG_B) / 12.0)
    k = hdr_light(name)[1]
    if name == "pq":
        p = _pow_host(c, k[0], dt)
        return _pow_host(np.maximum(p - k[1], dt(0.0)) * (dt(1.0) / (k[2] - k[3] * p)), k[4], dt)
    return np.where(c <= dt(0.5), (c * c) * k[0], (np.exp2((c - k[2]) * k[1]) + k[3]) * k[4])


def hdr_encode_host(lum, name, dtype=np.float64):
    """encode(L) of an HDR light, element-wise in `dtype`; as hdr_decode_host.  pq takes L <= 0 to c = 0 (include/ssm_hip.h says why)."""
    dt = np.dtype(dtype).type
    lum = np.asarray(lum, dtype=dt)
    with np.errstate(invalid="ignore", divide="ignore"):
        if dt is np.float64:
            if name == "pq":
                y = np.power(np.maximum(lum, 0.0), PQ_M1)
                return np.where(lum <= 0.0, 0.0, np.power((PQ_C1 + PQ_C2 * y) / (1.0 + PQ_C3 * y), PQ_M2))
            return np.where(lum <= 1.0 / 12.0, np.sqrt(3.0 * np.maximum(lum, 0.0)), HLG_A * np.log(12.0 * lum - HLG_B) + HLG_CC)
        k = hdr_light(name)[1]
        if name == "pq":
            y = _pow_host(np.maximum(lum, dt(0.0)), k[5], dt)
            return np.where(lum <= dt(0.0), dt(0.0), _pow_host((k[1] + k[2] * y) * (dt(1.0) / (dt(1.0) + k[3] * y)), k[6], dt))
        return np.where(lum <= k[4], np.sqrt(dt(3.0) * np.maximum(lum, dt(0.0))), k[5] * np.log2(dt(12.0) * lum - k[3]) + k[2])


def accumulate_hdr_host(frames, acc, init, scale, mean, std, name, encode, dtype=np.float64, weights=None):
    """Yardstick of ssm_frames_accumulate_hdr_fwd: accumulate_light_host with hdr_decode_host / hdr_encode_host of `name` ("pq", "hlg") in
    place of a curve's row - the same black comparison, clamp, order of the sum, scale and closing normalisation, in `dtype`.
    dtype = float64: the fixed point the kernel is held to within the bound of tests/test_video_hdr_cpu.py.  dtype = float32: plain fp32
    arithmetic in the kernel's steps; not the kernel bit for bit, whose log2, exp2, reciprocal and square root are the hardware's.
    weights: as accumulate_light_host's, the yardstick of ssm_frames_accumulate_hdr_weighted_fwd."""
    dt = np.dtype(dtype).type
    assert dt in (np.float32, np.float64), "dtype is numpy's float32 or float64"
    assert name in HDR_KINDS, "an HDR light is one of %s" % ", ".join(HDR_LIGHTS)
    frames = np.asarray(frames, dtype=_F)
    assert acc.dtype == dt and frames.ndim == 4 and frames.shape[0] >= 1 and frames.shape[1] == 3 and init in (0, 1, False, True) and \
        encode in (0, 1, False, True)
    dst = acc[0] if acc.ndim == 4 else acc
    assert dst.shape == frames.shape[1:] and (acc.ndim == 3 or acc.shape[0] == 1)
    m32, s32 = np.asarray(mean, dtype=_F).reshape(3, 1, 1), np.asarray(std, dtype=_F).reshape(3, 1, 1)
    black = (_F(0.0) / _F(255.0) - m32) / s32
    m, sd = m32.astype(dt), s32.astype(dt)

    def dec(v):
        c = np.where(v <= black, dt(0.0), np.clip(v.astype(dt) * sd + m, dt(0.0), dt(1.0)))
        return hdr_decode_host(c, name, dt)

    if weights is None:
        s = dec(frames[0]) if init else dst + dec(frames[0])
        for n in range(1, frames.shape[0]):
            s = s + dec(frames[n])
    else:
        w = _call_weights(weights, frames.shape[0], dt)
        s = w[0] * dec(frames[0]) if init else dst + w[0] * dec(frames[0])
        for n in range(1, frames.shape[0]):
            s = s + w[n] * dec(frames[n])
    r = s * dt(scale)
    dst[...] = (hdr_encode_host(r, name, dt) - m) / sd if encode else r
    return acc


def luma_sad_host(ya, yb):
    """Yardstick of ssm_luma_sad_fwd: uint8 Y planes [N,h,w] (numpy) -> uint64 [N], sums[n] = sum of |ya[n] - yb[n]| over the plane, exact."""
    ya, yb = np.asarray(ya), np.asarray(yb)
    assert ya.dtype == np.uint8 and yb.dtype == np.uint8 and ya.ndim == 3 and ya.shape == yb.shape
    return np.abs(ya.astype(np.int64) - yb.astype(np.int64)).reshape(ya.shape[0], -1).sum(axis=1).astype(np.uint64)


# ---- the kernels -------------------------------------------------------------------------------------------------------------------
class Clip:
    """A clip's format and what its two conversions need, worked out once per run: fb = frame_bytes, the canvas (hp, wp) = padded_dims(h, w,
    mult) unless `canvas` gives one, the centred offsets, mean, std and the bit depth's table as the C arrays the entry points take; dev: the
    run's device.  ingest() and egress() queue the kernel on the current stream and assert nothing of their tensors: the caller's to keep.
    window = (w', h', x, y), a checked rectangle of the h x w frame (letterboxed clips): h, w, the canvas and both conversions are then the
    window's, `frame` keeps the frame's (h, w); fb_in = fb is the frame's size, what comes up from the host, fb_out the window's, what goes
    back.  ingest() then queues ssm_window_cut_fwd into `scratch` ([N, fb_out], the caller's, per stream) and the conversion on that.
    Without a window fb_in = fb_out = fb and nothing changes."""

    def __init__(self, h, w, siting, matrix, crange, cfg=None, bits=8, mult=32, canvas=None, dev=None, window=None):
        self.frame, self.window, self.siting, self.bits = (h, w), window, siting, bits
        self.fb = self.fb_in = self.fb_out = frame_bytes(h, w, siting, bits)
        if window is not None:
            w, h = check_active(window, h, w, siting)[:2]
            self.fb_out = frame_bytes(h, w, siting, bits)
        self.h, self.w, self.dev = h, w, dev
        self.hp, self.wp = padded_dims(h, w, mult)[0] if canvas is None else canvas
        self.at = ((self.hp - h) // 2, (self.wp - w) // 2)          # top, left
        self.norm = tuple(_f3(v) for v in cfg_mean_std(cfg))          # mean, std
        self.coding = (_table_ptr(bits, matrix), table_index(matrix), crange, siting, sample_bytes(bits))          # the tail of both argument lists

    def ingest(self, payload, out, pad_before_norm=True, scratch=None):
        if self.window is not None:
            payload = window_cut(payload, *self.frame, self.siting, self.bits, self.window, out=scratch)
        hb.check(hb.load().ssm_frames_from_yuvx_fwd(payload.data_ptr(), hb.view_of(out), payload.shape[0], self.h, self.w, self.hp, self.wp,
                                                    *self.at, *self.norm, 1 if pad_before_norm else 0, *self.coding, hb.stream_ptr()))
        return out

    def egress(self, x, out):
        hb.check(hb.load().ssm_frames_to_yuvx_fwd(hb.view_of(x), out.data_ptr(), x.shape[0], self.h, self.w, *self.at, *self.norm, *self.coding,
                                                  hb.stream_ptr()))
        return out


def frames_from_yuv(payload, h, w, siting=CENTRED, matrix=BT709, color_range=LIMITED, cfg=None, pad_before_norm=True, out=None, multiple=32,
                    *, bits=8):
    """[N, frame_bytes] uint8 device tensor of Y4M payloads -> [N,3,Hp,Wp] normalised fp32 (into `out` if given); (Hp, Wp) =
    padded_dims(h, w, multiple): 32 for the path itself, 32 * flow_scale for the coarse-flow mode.  bits > 8: the bytes are 16-bit
    little-endian samples (a payload that does not start on an even address is refused)."""
    assert payload.is_cuda and payload.dtype == torch.uint8 and payload.dim() == 2 and payload.is_contiguous() and \
        payload.shape[1] == frame_bytes(h, w, siting, bits), "payloads must be a contiguous [N, frame_bytes] uint8 tensor on the GPU"
    clip = Clip(h, w, siting, matrix, color_range, cfg, bits, multiple)
    if out is None:
        out = torch.empty(payload.shape[0], 3, clip.hp, clip.wp, dtype=torch.float32, device=payload.device)
    assert tuple(out.shape) == (payload.shape[0], 3, clip.hp, clip.wp)
    return clip.ingest(payload, out, pad_before_norm)


def frames_to_yuv(x, h, w, siting=CENTRED, matrix=BT709, color_range=LIMITED, cfg=None, out=None, *, bits=8):
    """[N,3,Hp,Wp] normalised fp32 (finite) -> [N, frame_bytes] uint8 payloads (bits > 8: of 16-bit little-endian samples), the centred
    padding cropped away."""
    hb.require_device(x, "frame tensor")
    clip = Clip(h, w, siting, matrix, color_range, cfg, bits, canvas=x.shape[2:])
    if out is None:
        out = torch.empty(x.shape[0], clip.fb, dtype=torch.uint8, device=x.device)
    assert out.is_contiguous() and tuple(out.shape) == (x.shape[0], clip.fb) and out.dtype == torch.uint8
    return clip.egress(x, out)


def _pair_operands(payload_a, payload_b, row_bytes, row_name, out, per_pair):
    """What the calls on two sets of payloads (luma_sad here, video_score.plane_sse and plane_ssim) ask of their tensors: [N, at least
    row_bytes] uint8 on the GPU with unit stride within a row, as many rows in a as in b, on one device.  -> (N, `out`: a contiguous int64
    [N, *per_pair] on the device, made if None, and the two row strides as the entry points take them).  The stride of a single row names
    nothing: with N = 1 it goes as 0, which every entry takes."""
    for t in (payload_a, payload_b):
        assert t.is_cuda and t.dtype == torch.uint8 and t.dim() == 2 and t.shape[1] >= row_bytes and (t.shape[1] == 1 or t.stride(1) == 1), \
            "payloads must be [N, at least %s] uint8 tensors on the GPU with unit stride within a frame" % row_name
    n = payload_a.shape[0]
    assert payload_b.shape[0] == n and payload_b.device == payload_a.device, "as many frames in a as in b, on one device"
    if out is None:
        out = torch.empty((n,) + per_pair, dtype=torch.int64, device=payload_a.device)
    assert out.is_cuda and out.dtype == torch.int64 and tuple(out.shape) == (n,) + per_pair and out.is_contiguous()
    sa, sb = (t.stride(0) if n > 1 else 0 for t in (payload_a, payload_b))
    return n, out, sa, sb


def luma_sad(payload_a, payload_b, h, w, out=None):
    """ssm_luma_sad_fwd on payloads: [N, frame_bytes] uint8 device tensors (rows of at least h * w bytes, unit stride within a row, any
    row stride: views of one buffer, frames n and n + 1, are fine) -> int64 [N] on the device (into `out` if given), out[n] = the sum
    over the h x w Y planes of |a_n - b_n|.  The words are unsigned and below 2^63: read them on the host as numpy uint64."""
    n, out, sa, sb = _pair_operands(payload_a, payload_b, h * w, "h * w", out, ())
    hb.check(hb.load().ssm_luma_sad_fwd(payload_a.data_ptr(), payload_b.data_ptr(), sa, sb, n, h, w, out.data_ptr(), hb.stream_ptr()))
    return out


# ---- interlaced clips: fields ----------------------------------------------------------------------------------------------------------
TOP, BOTTOM = 0, 1                              # a field's parity: the rows of every plane of the frame it holds
FIELD_ORDERS = {"t": "tff", "b": "bff"}         # the Y4M header's I tag -> field order; tff: a frame's top field is the earlier one
DEINTERLACE = ("auto", "tff", "bff")


def field_dims(h, w, siting, what="an interlaced frame"):
    """(h / 2, w) of the fields of an h x w frame: h is even, and for the two 4:2:0 layouts a multiple of 4, so that both chroma fields
    have h / 4 rows; anything else is refused by name."""
    if h % 2:
        raise Y4MError("%s has an even number of rows: H=%d is odd" % (what, h))
    if siting in (CENTRED, COSITED) and h % 4:
        raise Y4MError("%s in 4:2:0 has a multiple of 4 rows, two chroma fields of H/4: H=%d is not" % (what, h))
    return h // 2, w


def split_fields_host(frames, h, w, siting=CENTRED, bits=8):
    """Yardstick of ssm_fields_split_fwd: [N, frame_bytes(h, w)] uint8 (numpy) -> [2N, frame_bytes(h / 2, w)] uint8, the top field of frame
    n (the even rows of every plane) at 2n and its bottom field (the odd rows) at 2n + 1.  Storage order is by parity, not by time."""
    fh, _ = field_dims(h, w, siting)
    frames = np.ascontiguousarray(frames).reshape(-1, frame_bytes(h, w, siting, bits))
    out = np.empty((2 * frames.shape[0], frame_bytes(fh, w, siting, bits)), np.uint8)
    for src, dst in zip(split_planes(frames, h, w, siting, bits), split_planes(out, fh, w, siting, bits)):
        dst[0::2], dst[1::2] = src[:, 0::2], src[:, 1::2]
    return out


def weave_fields_host(kept, made, h, w, siting=CENTRED, bits=8, parity0=TOP, fill=0):
    """Yardstick of ssm_fields_weave_fwd: kept, made [N, frame_bytes(h / 2, w)] uint8 (numpy) -> [N, frame_bytes(h, w)] uint8.  Frame n has
    kept[n] on its rows of parity (parity0 + n) & 1 of every plane.  fill = 0: made[n] on the other rows.  fill = 1 (made is not looked
    at): a missing row y of a plane is (a + b + 1) >> 1 per sample, in integers, a = kept row y - 1 and b = kept row y + 1 of the frame's
    plane; where one of them lies outside the plane, both are the other one."""
    assert parity0 in (0, 1) and fill in (0, 1)
    fh, _ = field_dims(h, w, siting)
    kept = np.ascontiguousarray(kept).reshape(-1, frame_bytes(fh, w, siting, bits))
    out = np.empty((kept.shape[0], frame_bytes(h, w, siting, bits)), np.uint8)
    made = [None] * 3 if fill else split_planes(np.ascontiguousarray(made).reshape(kept.shape), fh, w, siting, bits)
    for k, m, dst in zip(split_planes(kept, fh, w, siting, bits), made, split_planes(out, h, w, siting, bits)):
        for n in range(kept.shape[0]):
            own = (parity0 + n) & 1
            dst[n, own::2] = k[n]
            if not fill:
                dst[n, 1 - own::2] = m[n]
                continue
            wide = k[n].astype(np.uint32)
            up, down = (wide, np.concatenate([wide[1:], wide[-1:]])) if own == TOP else (np.concatenate([wide[:1], wide[:-1]]), wide)
            dst[n, 1 - own::2] = ((up + down + 1) >> 1).astype(dst.dtype)
    return out


def _field_operand(t, n, row, name):
    assert t.is_cuda and t.dtype == torch.uint8 and t.dim() == 2 and t.shape[0] == n and t.shape[1] >= row and (t.shape[1] == 1 or t.stride(1) == 1), \
        "%s must be a [%d, at least %d] uint8 tensor on the GPU with unit stride within a payload" % (name, n, row)
    return t.stride(0) if n > 1 else 0


def fields_split(frames, h, w, siting=CENTRED, bits=8, out=None):
    """ssm_fields_split_fwd: a contiguous [N, frame_bytes(h, w)] uint8 device tensor -> [2N, frame_bytes(h / 2, w)] (into `out`, contiguous,
    if given): frame n's top field at 2n, its bottom field at 2n + 1."""
    fb = frame_bytes(h, w, siting, bits)
    assert frames.is_cuda and frames.dtype == torch.uint8 and frames.dim() == 2 and frames.shape[1] == fb and frames.is_contiguous(), \
        "frames must be a contiguous [N, frame_bytes] uint8 tensor on the GPU"
    n = frames.shape[0]
    if out is None:
        out = torch.empty(2 * n, fb // 2, dtype=torch.uint8, device=frames.device)
    assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (2 * n, fb // 2) and out.is_contiguous()
    hb.check(hb.load().ssm_fields_split_fwd(frames.data_ptr(), out.data_ptr(), n, h, w, siting, sample_bytes(bits), hb.stream_ptr()))
    return out


def fields_weave(kept, made, h, w, siting=CENTRED, bits=8, parity0=TOP, fill=0, out=None):
    """ssm_fields_weave_fwd: kept, made [N, at least frame_bytes(h / 2, w)] uint8 device tensors (unit stride within a payload, any row
    stride; made None with fill = 1) -> [N, at least frame_bytes(h, w)] (into `out` if given), as weave_fields_host."""
    fb = frame_bytes(h, w, siting, bits)
    n = kept.shape[0]
    sk = _field_operand(kept, n, fb // 2, "kept")
    sm = 0 if made is None else _field_operand(made, n, fb // 2, "made")
    if out is None:
        out = torch.empty(n, fb, dtype=torch.uint8, device=kept.device)
    so = _field_operand(out, n, fb, "out")
    hb.check(hb.load().ssm_fields_weave_fwd(kept.data_ptr(), sk, None if made is None else made.data_ptr(), sm, out.data_ptr(), so, n, h, w, siting,
                                            sample_bytes(bits), parity0, fill, hb.stream_ptr()))
    return out


def parse_deinterlace(value):
    """None, "auto", "tff" or "bff", as given; anything else is refused by name."""
    if value is not None and value not in DEINTERLACE:
        raise ValueError("unknown deinterlace %r: it is one of %s" % (value, ", ".join(DEINTERLACE)))
    return value


def field_order(deinterlace, interlace):
    """The field order of a run, "tff" or "bff": what deinterlace says, or with "auto" what the header's I tag says - Ip and I? are then
    refused (ffmpeg writes Ip for interlaced material whose order it does not know: say tff or bff)."""
    if deinterlace != "auto":
        return deinterlace
    if interlace not in FIELD_ORDERS:
        raise ValueError("deinterlace=\"auto\" takes the field order from the Y4M header, and this one says I%s: give deinterlace=\"tff\" or "
                         "\"bff\" for interlaced material whose header does not say" % interlace)
    return FIELD_ORDERS[interlace]


def field_of(f, order):
    """(frame, parity) of field g_f, the field at time f: frame f // 2 holds fields 2m and 2m + 1, under tff the top one first."""
    assert order in ("tff", "bff")
    return f // 2, (f & 1) ^ (1 if order == "bff" else 0)


def field_outputs(n, order):
    """The 2n output frames of an n-frame interlaced clip: per output f, (kept, left, right) as (frame, parity) each.  kept = g_f, whose
    bytes are the rows of its parity; the other rows come from the field synthesised at t = 1/2 between left = g_f-1 and right = g_f+1,
    which have the other parity - the missing rows' own; left = right = None for f = 0 and f = 2n - 1, whose missing rows are line
    averages of the kept field (fill = 1)."""
    out = []
    for f in range(2 * n):
        inner = 0 < f < 2 * n - 1
        out.append((field_of(f, order), field_of(f - 1, order) if inner else None, field_of(f + 1, order) if inner else None))
    return out


# ---- interlaced clips: the field order from the data --------------------------------------------------------------------------------------
# The definition is in include/ssm_hip.h and DESIGN 3.12: per frame the comb sums A0, A1, D of its luma plane against the frame before and
# the frame after, the kind of the frame from them, the verdict of a probe from the kinds.  The ratios are conventions in the spirit of
# ffmpeg's idet, not its construction: nothing claims its decisions frame for frame, and nothing was measured on compressed footage.
FIELD_PROBE = 48                   # frames the field order is decided on
FIELD_KINDS = "TBPU"               # top field first, bottom field first, progressive in motion, undetermined


def parse_field_probe(value):
    """The number of frames the field order is decided on: a whole number of at least 1, or its text."""
    try:
        n = int(value.strip()) if isinstance(value, str) else value
        if isinstance(n, bool) or int(n) != n or n < 1:
            raise ValueError
    except (ValueError, TypeError):
        raise ValueError("field_probe, the frames the field order is decided on, is a whole number of at least 1 (got %r)" % (value,)) from None
    return int(n)


def field_order_sums_host(prev, cur, nxt, h, w, bits=8):
    """Yardstick of ssm_field_order_sums_fwd: payloads prev, cur, nxt [N, at least h * w samples] uint8 (numpy; any of them may have a
    single row) -> uint64 [N, 3], out[n] = (A0, A1, D) of the luma planes, exact; with bits > 8 over the 16-bit words.  h < 3: zeros."""
    p, c, n = (_luma_of(x, h, w, bits) for x in (prev, cur, nxt))
    count = max(p.shape[0], c.shape[0], n.shape[0])
    p, c, n = (np.broadcast_to(x, (count, h, w)) for x in (p, c, n))
    if h < 3:
        return np.zeros((count, 3), np.uint64)
    s = c[:, :-2] + c[:, 2:]                                                              # rows y = 1 .. h - 2
    ep, en, ec = (np.abs(s - 2 * r[:, 1:-1]).sum(axis=2) for r in (p, n, c))          # [N, h - 2], row y at index y - 1
    even, odd = slice(1, None, 2), slice(0, None, 2)
    a0 = ep[:, even].sum(axis=1) + en[:, odd].sum(axis=1)
    a1 = ep[:, odd].sum(axis=1) + en[:, even].sum(axis=1)
    return np.stack([a0, a1, ec.sum(axis=1)], axis=1).astype(np.uint64)


def field_kind(a0, a1, d):
    """The kind of a frame from its comb sums, in integers: "T" if 25 A0 > 26 A1, else "B" if 25 A1 > 26 A0, else "P" (progressive, in
    motion) if 2 min(A0, A1) > 3 D, else "U"."""
    a0, a1, d = int(a0), int(a1), int(d)
    if 25 * a0 > 26 * a1:
        return "T"
    if 25 * a1 > 26 * a0:
        return "B"
    return "P" if 2 * min(a0, a1) > 3 * d else "U"


class FieldVerdict:
    """The decision over a probe: `kinds`, the kinds of its INNER frames 1 .. m - 2 (a frame needs the one before and the one after) as a
    string over FIELD_KINDS; `counts` = (nT, nB, nP, nU); `verdict` = "tff" if 2 nT > d, "bff" if 2 nB > d, "progressive" if 2 nP > d with
    d = nT + nB + nP, else None - also for a probe of fewer than 3 frames, which has no inner frame; `note`, one line with the counts."""
    NAMES = (("T", "tff"), ("B", "bff"), ("P", "progressive"))

    def __init__(self, kinds):
        self.kinds = "".join(kinds)
        assert set(self.kinds) <= set(FIELD_KINDS)
        self.counts = tuple(self.kinds.count(k) for k in FIELD_KINDS)
        d = sum(self.counts[:3])
        self.verdict = None
        for (_, name), n in zip(self.NAMES, self.counts):
            if 2 * n > d:
                self.verdict = name
        self.note = "field probe: %d inner frames, %d top field first, %d bottom field first, %d progressive, %d undetermined: %s" % (
            (len(self.kinds),) + self.counts + ("no verdict" if self.verdict is None else self.verdict,))

    @classmethod
    def of_sums(cls, sums):
        """From the [m - 2, 3] comb sums of a probe's inner frames."""
        return cls(field_kind(*row) for row in np.asarray(sums).reshape(-1, 3).tolist())


def field_order_sums(prev, cur, nxt, h, w, bits=8, out=None):
    """ssm_field_order_sums_fwd on payloads: three [N, at least h * w samples] uint8 device tensors (unit stride within a row, any row
    stride: frames n - 1, n, n + 1 of one buffer are fine) -> int64 [N, 3] on the device (into `out` if given): per frame (A0, A1, D), the
    comb sums of `cur` against `prev` and `nxt`.  The words are unsigned and below 2^63: read them on the host as numpy uint64."""
    sb = sample_bytes(bits)
    n, out, sp, sc = _pair_operands(prev, cur, h * w * sb, "h * w samples", out, (3,))
    _, _, _, sn = _pair_operands(cur, nxt, h * w * sb, "h * w samples", out, (3,))
    hb.check(hb.load().ssm_field_order_sums_fwd(prev.data_ptr(), cur.data_ptr(), nxt.data_ptr(), sp, sc, sn, n, h, w, sb, out.data_ptr(),
                                                hb.stream_ptr()))
    return out


# ---- the readers in front of the loop -----------------------------------------------------------------------------------------------------
FORMAT_ATTRS = ("width", "height", "siting", "chroma", "color_range", "aspect", "xtags", "frame_bytes", "rate")          # a reader's, mirrored


class LookAheadSource:
    """What FieldOrderSource, TelecineSource, RepeatSource and ActiveSource share: a reader that wraps a Y4MReader (or anything with its
    attributes, another source for one), reads the clip a chunk ahead of the loop, measures the chunk on the GPU, decides on the host and
    hands frames on.  It has the reader's format attributes (FORMAT_ATTRS, bits, extended, sample_bytes, interlace; field_order and
    field_bytes with fields=True, else None), frames_read (frames handed out), close() and the context manager.

    A chunk is `rows` new frames behind `carry` carried frames of the chunk before, in one pinned buffer, and behind the last `dev_carry` of
    those in one device buffer; both are made once (_window), with the results on the device and pinned.  Per chunk, on a stream of its
    own (_measure): one H2D, one kernel entry, one D2H per result tensor, one event wait; never a wait per frame.  _fill reads a chunk and
    carries, _probe reads the frames a decision is taken on and keeps them for replay, read_frame_into hands out the replayed frames,
    then what the source's _ahead() left in _pending (_take) or, with _straight, the reader's frames as they come."""
    _straight = False          # True: the frames behind the replayed ones come straight from the reader, nothing looks at them

    def __init__(self, reader, dev, takes, fields=False):
        self.reader, self.dev = reader, torch.device(dev)
        if self.dev.type != "cuda":
            raise RuntimeError("%s on the GPU (the HIP path has no CPU fallback)" % takes)
        for name in FORMAT_ATTRS:
            setattr(self, name, getattr(reader, name))
        self.bits, self.extended = getattr(reader, "bits", 8), getattr(reader, "extended", False)
        self.sample_bytes = sample_bytes(self.bits)
        self.interlace = getattr(reader, "interlace", "p")
        self.field_order, self.field_bytes = (getattr(reader, "field_order", None), getattr(reader, "field_bytes", None)) if fields else (None, None)
        self.frames_read = 0
        self._replay, self._pending, self._eof = [], [], False          # probed frames; what _take hands out next; the reader has ended
        self._base = None          # the clip's frame in row 0 of the pinned buffer (below 0 in the first chunk); None before it
        self._np = None

    def _window(self, rows, carry, dev_carry, results):
        """The buffers of a chunk: pinned [carry + rows, frame_bytes] (_np its numpy view), device [dev_carry + rows, frame_bytes], and per
        (trailing shape, dtype) of `results` a [rows, ...] tensor on the device and a pinned one, read on the host as unsigned words."""
        self._rows, self._carry = rows, carry
        self._host = torch.empty(carry + rows, self.frame_bytes, dtype=torch.uint8).pin_memory()
        self._np = self._host.numpy()
        self._dev = torch.empty(dev_carry + rows, self.frame_bytes, dtype=torch.uint8, device=self.dev)
        self._dev_results = [torch.empty((rows,) + tuple(shape), dtype=dtype, device=self.dev) for shape, dtype in results]
        self._host_results = [torch.empty(t.shape, dtype=t.dtype).pin_memory() for t in self._dev_results]
        self._np_results = [t.numpy().view("u%d" % t.element_size()) for t in self._host_results]
        self._stream, self._event = torch.cuda.Stream(self.dev), torch.cuda.Event()

    def _measure(self, k, rows, launch):
        """The pinned rows of the slice `rows` to the front of the device buffer, launch(those device rows, the first k rows of every
        device result), the results back: per result its first k rows, unsigned, views of pinned memory that the next call overwrites."""
        dev = self._dev[:rows.stop - rows.start]
        with torch.cuda.stream(self._stream):
            dev.copy_(self._host[rows], non_blocking=True)
            launch(dev, *(t[:k] for t in self._dev_results))
            for hr, dr in zip(self._host_results, self._dev_results):
                hr[:k].copy_(dr[:k], non_blocking=True)
            self._event.record()
        self._event.synchronize()
        return [r[:k] for r in self._np_results]

    def _fill(self):
        """The next chunk: up to `rows` frames of the reader into the pinned buffer behind the carried ones -> how many; fewer than `rows`
        is the end of the clip (_eof).  A source that carries has the clip's first frame in its last carried row, so that every new row
        has the row before it, and refuses a stream without one."""
        rows, c = self._rows, self._carry
        if self._base is None:
            if c and not self.reader.read_frame_into(self._np[c - 1]):
                raise Y4MError("the Y4M stream holds no frame")
            self._base = 1 - c if c else 0
        else:
            self._base += rows          # a chunk that is not the last one is full
            self._np[:c] = self._np[rows:rows + c].copy()          # the two overlap where rows < carry
        k = 0
        while k < rows and self.reader.read_frame_into(self._np[c + k]):
            k += 1
        self._eof = k < rows
        return k

    def _probe(self, n):
        """The first n frames of the reader (or the whole clip if it is shorter) [m, frame_bytes], kept to be handed out first."""
        probe = np.empty((n, self.frame_bytes), np.uint8)
        m = 0
        while m < n and self.reader.read_frame_into(probe[m]):
            m += 1
        self._eof = m < n
        self._replay = [probe[i] for i in range(m)]
        return probe[:m]

    def _ahead(self):
        """Before a frame is handed out: the source decides, or reads chunks until _pending holds what it needs or the clip has ended."""

    def _take(self, n, out):
        """Hands out an entry of _pending: clip frame n, a row of the pinned buffer."""
        out[:] = self._np[n - self._base]

    def read_frame_into(self, buf):
        """The next frame's payload into `buf`; False at the end of the clip."""
        self._ahead()
        out = np.frombuffer(memoryview(buf).cast("B"), np.uint8)
        if out.size != self.frame_bytes:
            raise ValueError("buffer of %d bytes for frames of %d" % (out.size, self.frame_bytes))
        if self._replay:
            out[:] = self._replay.pop(0)
        elif self._pending:
            self._take(self._pending.pop(0), out)
        elif self._eof or not self._straight or not self.reader.read_frame_into(out):
            self._eof = True
            return False
        self.frames_read += 1
        return True

    def close(self):
        self.reader.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class FieldOrderSource(LookAheadSource):
    """A reader that probes the field order of a clip and hands out the wrapped reader's frames as they are.  decide() reads the first
    `probe` frames (or the whole clip if it is shorter), takes the comb sums of the inner ones on the GPU, and sets `kinds`, `counts`,
    `verdict` ("tff", "bff", "progressive" or None: FieldVerdict) and `note`, one log line with the four counts; then the probed frames are
    replayed, and the frames behind the probe come straight from the reader: nothing watches them.

    A chunk carries two frames, on the host and on the device: ssm_field_order_sums_fwd takes the frame before, the frame and the frame
    after as rows b - 1, b, b + 1 of the device buffer, one pointer each and one stride.  The bytes handed out are the reader's; neither
    they nor the verdict depend on frames_per_chunk."""
    _straight = True

    def __init__(self, reader, dev, probe=FIELD_PROBE, frames_per_chunk=8):
        assert frames_per_chunk >= 1
        super().__init__(reader, dev, "the field probe takes its comb sums", fields=True)
        self.probe = parse_field_probe(probe)
        self.kinds = self.counts = self.verdict = self.note = None
        self._rows, self._decided = frames_per_chunk, False

    def _sums(self, frames):
        """The comb sums of frames 1 .. m - 2 of `frames` [m, frame_bytes]: uint64 [m - 2, 3]."""
        m, c, h, w = frames.shape[0], self._rows, self.height, self.width
        self._window(c, 2, 2, [((3,), torch.int64)])
        out = np.zeros((max(m - 2, 0), 3), np.uint64)
        for at in range(0, m, c):          # the chunk's new frames are at .. at + k - 1; it closes the inner frames whose next frame is new
            k, lo = min(c, m - at), max(0, at - 2)
            first, last = max(1, at - 1), at + k - 2
            if last < first:
                continue
            cnt, b = last - first + 1, first - lo
            self._np[:at + k - lo] = frames[lo:at + k]
            (sums,) = self._measure(cnt, slice(0, at + k - lo), lambda dev, res: field_order_sums(
                dev[b - 1:b - 1 + cnt], dev[b:b + cnt], dev[b + 1:b + 1 + cnt], h, w, self.bits, out=res))
            out[first - 1:last] = sums
        # nothing is measured behind the probe: the buffers go back to the allocators, where the run's pinned ring finds them
        self._host = self._np = self._dev = self._dev_results = self._host_results = self._np_results = None
        return out

    def decide(self):
        """The verdict of the probe: "tff", "bff", "progressive" or None.  Reads the probe frames on the first call."""
        if not self._decided:
            self._decided = True
            self.sums = self._sums(self._probe(self.probe))
            v = FieldVerdict.of_sums(self.sums)
            self.kinds, self.counts, self.verdict, self.note = v.kinds, v.counts, v.verdict, v.note
        return self.verdict

    _ahead = decide


# ---- YUV4MPEG2 ---------------------------------------------------------------------------------------------------------------------
class Y4MError(ValueError):
    pass


def _ratio(text, what):
    try:
        a, b = text.split(":")
        return int(a), int(b)
    except ValueError:
        raise Y4MError("bad %s %r in the Y4M header" % (what, text)) from None


class Y4MReader:
    """A YUV4MPEG2 stream from a path, `-` (stdin) or a binary file object.  Attributes: width, height, rate (num, den), interlace,
    aspect (num, den), chroma (the C tag's text, `420jpeg` when absent), siting, bits, sample_bytes, color_range (LIMITED / FULL from
    ffmpeg's XCOLORRANGE tag, None when absent), xtags (every X tag as read), frame_bytes.  extended=True: EXTENDED_TAGS (4:2:2 and 9 to
    16 bits per sample) beside the 8-bit 4:2:0 and 4:4:4 tags that are taken without it.  interlaced=True: It and Ib are taken (Im and
    anything else unknown stay refused); field_order is then "tff" / "bff" (None for Ip and I?) and field_bytes the payload of one field,
    frame_bytes at H/2; a frame is still read whole.  Without it an interlaced header is refused, as ever."""

    def __init__(self, src, extended=False, interlaced=False):
        self.extended, self.interlaced = bool(extended), bool(interlaced)
        self._own = isinstance(src, str) and src != "-"
        self.f = open(src, "rb") if self._own else (sys.stdin.buffer if src == "-" else src)
        line = self.f.readline(4096)
        if not line.endswith(b"\n") or not line.startswith(b"YUV4MPEG2"):
            raise Y4MError("not a YUV4MPEG2 stream (no `YUV4MPEG2 ...` header line)")
        toks = line[:-1].decode("ascii", "replace").split(" ")
        if toks[0] != "YUV4MPEG2":
            raise Y4MError("not a YUV4MPEG2 stream (signature %r)" % toks[0])
        self.width = self.height = None
        self.rate, self.aspect, self.interlace, self.chroma, self.xtags = (25, 1), (0, 0), "p", "420jpeg", []
        for t in toks[1:]:
            if not t:
                continue
            key, val = t[0], t[1:]
            if key == "W":
                self.width = int(val)
            elif key == "H":
                self.height = int(val)
            elif key == "F":
                self.rate = _ratio(val, "frame rate")
            elif key == "A":
                self.aspect = _ratio(val, "pixel aspect")
            elif key == "I":
                self.interlace = val
            elif key == "C":
                self.chroma = val
            elif key == "X":
                self.xtags.append(val)
            else:
                raise Y4MError("unknown Y4M header field %r" % t)
        if not self.width or not self.height or self.width < 1 or self.height < 1:
            raise Y4MError("the Y4M header has no frame size (W, H)")
        if self.interlace not in ("p", "?") and not (self.interlaced and self.interlace in FIELD_ORDERS):
            raise Y4MError("interlaced Y4M input (I%s) is not supported: deinterlace first" % self.interlace)
        self.field_order = FIELD_ORDERS.get(self.interlace)
        self.siting, self.bits = chroma_format(self.chroma, self.extended)
        self.sample_bytes = sample_bytes(self.bits)
        self.color_range = None
        for x in self.xtags:
            if x.startswith("COLORRANGE="):
                v = x.split("=", 1)[1].lower()
                if v not in RANGES:
                    raise Y4MError("unknown XCOLORRANGE=%s in the Y4M header" % x.split("=", 1)[1])
                self.color_range = RANGES[v]
        self.frame_bytes = frame_bytes(self.height, self.width, self.siting, self.bits)
        self.field_bytes = None
        if self.field_order is not None:
            self.field_bytes = frame_bytes(*field_dims(self.height, self.width, self.siting, "interlaced Y4M input (I%s)" % self.interlace),
                                           self.siting, self.bits)
        self.frames_read = 0

    def read_frame_into(self, buf):
        """The next frame's payload into `buf` (writable, frame_bytes long; e.g. a row of a pinned tensor as numpy).  False at the end of
        the stream; a record cut short is an error, not the end."""
        line = self.f.readline(4096)
        if not line:
            return False
        if not line.endswith(b"\n") or not (line == b"FRAME\n" or line.startswith(b"FRAME ")):
            raise Y4MError("frame %d: expected a FRAME record, got %r" % (self.frames_read, line[:16]))
        mv = memoryview(buf).cast("B")
        if len(mv) != self.frame_bytes:
            raise ValueError("buffer of %d bytes for frames of %d" % (len(mv), self.frame_bytes))
        got = 0
        while got < len(mv):
            n = self.f.readinto(mv[got:])
            if not n:
                raise Y4MError("frame %d is truncated: %d of %d bytes" % (self.frames_read, got, len(mv)))
            got += n
        self.frames_read += 1
        return True

    def close(self):
        if self._own:
            self.f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class Y4MWriter:
    """Writes the stream header at once, then one FRAME record per write_frame().  extended=True: the tags of EXTENDED_TAGS, as the reader."""

    def __init__(self, dst, width, height, rate=(25, 1), aspect=(0, 0), chroma="420jpeg", color_range=None, interlace="p", xtags=(),
                 extended=False):
        self.extended = bool(extended)
        siting, self.bits = chroma_format(chroma, self.extended)
        self.sample_bytes = sample_bytes(self.bits)
        self._own = isinstance(dst, str) and dst != "-"
        self.f = open(dst, "wb") if self._own else (sys.stdout.buffer if dst == "-" else dst)
        self.width, self.height, self.rate, self.aspect, self.chroma = int(width), int(height), tuple(rate), tuple(aspect), chroma
        self.siting, self.color_range, self.interlace = siting, color_range, interlace
        self.xtags = [x for x in xtags if not x.startswith("COLORRANGE=")]
        if color_range is not None:
            self.xtags.append("COLORRANGE=" + ("FULL" if color_range == FULL else "LIMITED"))
        self.frame_bytes = frame_bytes(self.height, self.width, self.siting, self.bits)
        self.frames_written = 0
        head = "YUV4MPEG2 W%d H%d F%d:%d I%s A%d:%d C%s" % (self.width, self.height, self.rate[0], self.rate[1], interlace,
                                                            self.aspect[0], self.aspect[1], chroma)
        self.f.write((head + "".join(" X" + x for x in self.xtags) + "\n").encode("ascii"))

    @classmethod
    def like(cls, dst, reader, rate=None, color_range=None):
        """A writer for frames of `reader`'s format (its `extended` flag with it); `rate` and `color_range` override the reader's."""
        return cls(dst, reader.width, reader.height, rate or reader.rate, reader.aspect, reader.chroma,
                   reader.color_range if color_range is None else color_range, "p", reader.xtags, extended=getattr(reader, "extended", False))

    def write_frame(self, buf):
        mv = memoryview(buf).cast("B")
        if len(mv) != self.frame_bytes:
            raise ValueError("frame of %d bytes, the stream's frames have %d" % (len(mv), self.frame_bytes))
        self.f.write(b"FRAME\n")
        self.f.write(mv)
        self.frames_written += 1

    def close(self):
        self.f.flush()
        if self._own:
            self.f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


# ---- 3:2 pulldown removal ----------------------------------------------------------------------------------------------------------------
# The definition is in include/ssm_hip.h and DESIGN 3.12: film frames A B C D in five video frames, per pattern and cadence position q the
# film frames (by their place in the cycle) on a video frame's top and bottom rows.
PULLDOWN = (((0, 0), (1, 1), (1, 2), (2, 3), (3, 3)),          # pattern 0, top field first: the top field repeats at q = 2, the bottom at q = 4
            ((0, 0), (1, 1), (2, 1), (3, 2), (3, 3)))          # pattern 1, bottom field first
HYPOTHESES = 10                                                 # h = 5 * pattern + phi, frame n at q = (n - phi) % 5


def _luma_of(payload, h, w, bits):
    sb = sample_bytes(bits)
    payload = np.asarray(payload)
    assert payload.dtype == np.uint8 and payload.ndim == 2 and payload.shape[1] >= h * w * sb, "payloads are [N, at least the luma plane] uint8"
    y = np.ascontiguousarray(payload[:, :h * w * sb])
    return (y.view("<u2") if sb == 2 else y).reshape(-1, h, w).astype(np.int64)


def field_diff_host(a, b, h, w, bits=8):
    """Yardstick of ssm_field_diff_fwd: payloads a, b [N, at least h * w samples] uint8 (numpy; one of them may have a single row) ->
    uint64 [N, 2], out[n, p] = the sum over the luma rows of parity p of |a_n - b_n|, exact; with bits > 8 over the 16-bit words."""
    d = np.abs(_luma_of(a, h, w, bits) - _luma_of(b, h, w, bits))
    return np.stack([d[:, 0::2].reshape(d.shape[0], -1).sum(axis=1), d[:, 1::2].reshape(d.shape[0], -1).sum(axis=1)], axis=1).astype(np.uint64)


def field_diff(payload_a, payload_b, h, w, bits=8, out=None):
    """ssm_field_diff_fwd on payloads: [N, at least h * w samples] uint8 device tensors (unit stride within a row, any row stride: frames
    n + 1 and n of one buffer are fine) -> int64 [N, 2] on the device (into `out` if given): per pair the sums of |a_n - b_n| over the luma
    rows of parity 0 (the top fields) and 1 (the bottom fields).  The words are unsigned and below 2^63."""
    sb = sample_bytes(bits)
    n, out, sa, sb_stride = _pair_operands(payload_a, payload_b, h * w * sb, "h * w samples", out, (2,))
    hb.check(hb.load().ssm_field_diff_fwd(payload_a.data_ptr(), payload_b.data_ptr(), sa, sb_stride, n, h, w, sb, out.data_ptr(), hb.stream_ptr()))
    return out


def _weave_rows(dst, top, bottom, h, w, siting, bits):
    """dst = the rows of parity 0 of every plane of `top` and the rows of parity 1 of `bottom`: payloads of one frame, as numpy rows."""
    for d, t, b in zip(*(split_planes(p.reshape(1, -1), h, w, siting, bits) for p in (dst, top, bottom))):
        d[0, 0::2], d[0, 1::2] = t[0, 0::2], b[0, 1::2]


def telecine_host(film, h, w, siting=CENTRED, bits=8, pattern=0, phase=0):
    """3:2 pulldown of progressive payloads film [F, frame_bytes] (numpy) -> the video clip [n, frame_bytes]: frame m sits at cadence
    position q = (phase + m) % 5 of PULLDOWN[pattern] and weaves the rows of two film frames.  The clip is a cut out of the endless
    pulldown: film[0] is the first film frame any of its fields shows (A at phase 0, B at 1 and 2, C at 3, D at 4), and it ends before
    the first video frame that would need film[F].  The maker of test and benchmark clips."""
    assert pattern in (0, 1) and 0 <= phase < 5
    field_dims(h, w, siting, "a telecined frame")
    film = np.ascontiguousarray(film).reshape(-1, frame_bytes(h, w, siting, bits))
    first = min(PULLDOWN[pattern][phase])
    out = []
    for m in range(5 * len(film)):
        c, q = divmod(phase + m, 5)
        t, b = (4 * c + x - first for x in PULLDOWN[pattern][q])
        if max(t, b) >= len(film):
            break
        frame = np.empty_like(film[0])
        _weave_rows(frame, film[t], film[b], h, w, siting, bits)
        out.append(frame)
    return np.stack(out) if out else np.zeros((0, film.shape[1]), np.uint8)


class Cadence:
    """The cadence decision, in Python ints and free of the GPU.  feed(dT, dB) takes the field differences of the next frame n = 1, 2, ...
    against frame n - 1 and returns the frames that this closes, [] until a window of five is full: [(n, action)] with action None (the
    frame is dropped) or (t, b), the frames whose top rows and bottom rows make the output - (n, n) is the frame's own bytes, (n, n - 1)
    and (n - 1, n) the weaves of patterns 0 and 1 at q = 3.  Window 0 closes frames 0 .. 5, window j > 0 frames 5 j + 1 .. 5 j + 5; end()
    closes the frames after the last full window under the last hypothesis, and refuses a clip without a window.  `log`: per window (first
    frame, h, best score, second-best score); `dropped`: the frames dropped so far; `combed_first`: frame 0 sat at q = 3 and went out as it
    stands."""

    def __init__(self):
        self.h, self.log, self.dropped, self.combed_first = None, [], 0, False
        self._fed, self._window = 0, []

    @staticmethod
    def position(n, h):
        return (n - h % 5) % 5

    def _action(self, n):
        q, pattern = self.position(n, self.h), self.h // 5
        if q == 2:
            self.dropped += 1
            return n, None
        if q == 3 and n == 0:
            self.combed_first = True
        if q != 3 or n == 0:
            return n, (n, n)
        return n, ((n, n - 1) if pattern == 0 else (n - 1, n))

    def feed(self, dt, db):
        self._fed += 1
        self._window.append((int(dt), int(db)))
        if len(self._window) < 5:
            return []
        first = self._fed - 4
        at = {n: d for n, d in zip(range(first, first + 5), self._window)}
        scores = []
        for h in range(HYPOTHESES):
            n2, n4 = (next(n for n in at if self.position(n, h) == q) for q in (2, 4))
            scores.append(at[n2][h // 5] + at[n4][1 - h // 5])          # pattern 0: dT[n2] + dB[n4]; pattern 1: dB[n2] + dT[n4]
        best = min(scores)
        self.h = self.h if self.h is not None and scores[self.h] == best else scores.index(best)
        self.log.append((first, self.h, best, sorted(scores)[1]))
        self._window = []
        return [self._action(n) for n in range(0 if first == 1 else first, first + 5)]

    def end(self):
        if self.h is None:
            raise Y4MError("pulldown removal needs one cadence window, frames 1 .. 5 after frame 0: the clip has %d frames, fewer than 6"
                           % (self._fed + 1))
        tail, self._window = len(self._window), []
        return [self._action(n) for n in range(self._fed - tail + 1, self._fed + 1)]


def detelecine_rate(rate):
    """The output rate of pulldown removal, (num, den) reduced: four frames out per five in, 30000:1001 -> 24000:1001."""
    r = Fraction(4 * rate[0], 5 * rate[1])
    return r.numerator, r.denominator


def detelecine_host(frames, h, w, siting=CENTRED, bits=8):
    """The whole definition in numpy, the yardstick of TelecineSource: video payloads [n, frame_bytes] -> (the film payloads [m,
    frame_bytes], the Cadence that decided, for its log)."""
    field_dims(h, w, siting, "a telecined frame")
    frames = np.ascontiguousarray(frames).reshape(-1, frame_bytes(h, w, siting, bits))
    cadence, actions = Cadence(), []
    if len(frames) > 1:
        for dt, db in field_diff_host(frames[1:], frames[:-1], h, w, bits):
            actions += cadence.feed(dt, db)
    actions += cadence.end()
    out = []
    for n, act in actions:
        if act is not None:
            out.append(np.empty_like(frames[0]))
            _weave_rows(out[-1], frames[act[0]], frames[act[1]], h, w, siting, bits)
    return np.stack(out), cadence


class TelecineSource(LookAheadSource):
    """A reader that undoes 3:2 pulldown: wraps a reader of telecined video and hands out the film's frames, so that everything
    downstream sees a progressive clip at detelecine_rate(reader.rate).  It has interlace "p", frames_read (film frames handed out), and
    of the decision so far `cadence` (Cadence.log: per window its first frame, h, best and second-best score), `dropped` and
    `combed_first`.

    A chunk is 5 * windows_per_chunk new frames behind one carried frame: ssm_field_diff_fwd takes row n + 1 against row n, one stride
    each.  Three film frames in four are straight copies out of the pinned buffer, the fourth a row-strided numpy copy per plane.  The
    bytes handed out do not depend on windows_per_chunk."""

    def __init__(self, reader, dev, windows_per_chunk=2):
        assert windows_per_chunk >= 1
        super().__init__(reader, dev, "pulldown removal takes its field differences")
        field_dims(self.height, self.width, self.siting, "a telecined frame")
        self.interlace, self.rate = "p", detelecine_rate(reader.rate)
        self._cadence = Cadence()
        self._window(5 * windows_per_chunk, 1, 1, [((2,), torch.int64)])

    def _chunk(self):
        """The next chunk: its frames' field differences and what the cadence closes, as (top rows' frame, bottom rows' frame)."""
        k = self._fill()
        closed = []
        if k:
            (sums,) = self._measure(k, slice(0, k + 1), lambda dev, res: field_diff(dev[1:], dev[:-1], self.height, self.width, self.bits, out=res))
            for dt, db in sums:
                closed += self._cadence.feed(dt, db)
        if self._eof:
            closed += self._cadence.end()
        self._pending += [act for _, act in closed if act is not None]

    def _ahead(self):
        while not self._pending and not self._eof:
            self._chunk()

    def _take(self, act, out):
        t, b = act
        if t == b:
            out[:] = self._np[t - self._base]
        else:
            _weave_rows(out, self._np[t - self._base], self._np[b - self._base], self.height, self.width, self.siting, self.bits)

    cadence = property(lambda self: self._cadence.log)
    dropped = property(lambda self: self._cadence.dropped)
    combed_first = property(lambda self: self._cadence.combed_first)


# ---- repeated frames ------------------------------------------------------------------------------------------------------------------
# The definition is in include/ssm_hip.h and DESIGN 3.12: 8 x 8 blocks of every plane, per pair and plane the largest block sum of |a - b|
# and the number of blocks above `lo`; a frame repeats the one before iff every plane that has blocks stays within (hi, floor(frac blocks)).
# The numbers are ffmpeg's mpdecimate defaults at 8 bits (64 * 12, 64 * 5, 0.33), the construction is not: a convention.
DEDUP_HI, DEDUP_LO, DEDUP_FRAC = 768, 320, Fraction(33, 100)
DEDUP_MAX = 2                      # the longest run that is repaired: animation on threes, 2:3 repetition
BLOCK_SAD_MAX = 1 << 22            # above every block sum (64 * 65535): the largest `lo` ssm_block_sad_fwd takes


def block_counts(h, w, siting):
    """The 8 x 8 blocks of the Y, U and V plane of an h x w frame: (rows >> 3) * (cols >> 3) each; 0 for a plane below 8 rows or columns."""
    ch, cw = chroma_dims(h, w, siting)
    return ((h >> 3) * (w >> 3), (ch >> 3) * (cw >> 3), (ch >> 3) * (cw >> 3))


def parse_dedup(text=None):
    """The thresholds of the repeat test: "HI:LO:FRAC" (two integers >= 0 in codes of the clip's depth, LO at most 2^22, and a decimal or
    a fraction in [0, 1]: "768:320:0.33", "0:0:0" for exact repeats only), or such a triple -> (hi, lo, Fraction frac); None, "" or True
    -> True, the defaults DEDUP_HI, DEDUP_LO scaled to the clip's depth and DEDUP_FRAC (dedup_thresholds).  Anything else is a ValueError
    naming the value."""
    if text is None or text is True or (isinstance(text, str) and not text.strip()):
        return True
    try:
        hi, lo, frac = text.strip().split(":") if isinstance(text, str) else text
        if any(isinstance(x, bool) or (not isinstance(x, str) and int(x) != x) for x in (hi, lo)):
            raise ValueError
        hi, lo = int(hi), int(lo)
        frac = Fraction(frac.strip() if isinstance(frac, str) else frac)
    except (ValueError, TypeError, ZeroDivisionError):
        raise ValueError("the repeat thresholds are written HI:LO:FRAC, two integers and a decimal or a fraction, e.g. 768:320:0.33 or 0:0:0 "
                         "(got %r)" % (text,)) from None
    if hi < 0 or not 0 <= lo <= BLOCK_SAD_MAX or not 0 <= frac <= 1:
        raise ValueError("the repeat thresholds HI:LO:FRAC want HI >= 0, LO in 0 .. 2^22 and FRAC in [0, 1] (got %r)" % (text,))
    return hi, lo, frac


def dedup_thresholds(dedup, bits=8):
    """(hi, lo, frac) of a parsed `dedup` for samples of `bits` bits: the triple as given, or the defaults at that depth."""
    dedup = parse_dedup(dedup)
    return (DEDUP_HI << (bits - 8), DEDUP_LO << (bits - 8), DEDUP_FRAC) if dedup is True else dedup


def parse_dedup_max(value):
    if isinstance(value, bool) or int(value) != value or value < 1:
        raise ValueError("dedup_max, the longest run of repeats that is repaired, is a whole number of at least 1 (got %r)" % (value,))
    return int(value)


def parse_dedup_max_text(text):
    """parse_dedup_max of a command line's text."""
    try:
        return parse_dedup_max(int(str(text).strip()))
    except ValueError:
        raise ValueError("dedup_max, the longest run of repeats that is repaired, is a whole number of at least 1 (got %r)" % (text,)) from None


def block_sad_host(a, b, h, w, siting, bits=8, lo=None):
    """Yardstick of ssm_block_sad_fwd: payloads a, b [N, at least frame_bytes] uint8 (numpy; one of them may have a single row) -> uint64
    [N, 3, 2]: per pair and plane (Y, U, V) the largest 8 x 8 block sum of |a_n - b_n| and the number of blocks whose sum is above `lo`
    (None: the default DEDUP_LO at this depth); (0, 0) for a plane without blocks.  With bits > 8 over the 16-bit words."""
    lo = DEDUP_LO << (bits - 8) if lo is None else int(lo)
    fb = frame_bytes(h, w, siting, bits)
    planes = []
    for p in (a, b):
        p = np.asarray(p)
        assert p.dtype == np.uint8 and p.ndim == 2 and p.shape[1] >= fb, "payloads are [N, at least frame_bytes] uint8"
        planes.append(split_planes(np.ascontiguousarray(p[:, :fb]), h, w, siting, bits))
    n = max(planes[0][0].shape[0], planes[1][0].shape[0])
    out = np.zeros((n, 3, 2), np.uint64)
    for p, (x, y) in enumerate(zip(*planes)):
        by, bx = x.shape[1] >> 3, x.shape[2] >> 3
        if by and bx:
            d = np.abs(x[:, :8 * by, :8 * bx].astype(np.int64) - y[:, :8 * by, :8 * bx].astype(np.int64))
            d = d.reshape(d.shape[0], by, 8, bx, 8).sum(axis=(2, 4)).reshape(d.shape[0], -1)
            out[:, p, 0], out[:, p, 1] = d.max(axis=1), (d > lo).sum(axis=1)
    return out


def block_sad(payload_a, payload_b, h, w, siting, bits=8, lo=None, out=None):
    """ssm_block_sad_fwd on payloads: [N, at least frame_bytes] uint8 device tensors (unit stride within a row, any row stride: frames
    n + 1 and n of one buffer are fine; a single row goes against N) -> int64 [N, 3, 2] on the device (into `out` if given): per pair and
    plane the largest 8 x 8 block sum of |a_n - b_n| and the number of blocks above `lo` (None: DEDUP_LO at this depth).  The words are
    unsigned and below 2^63."""
    lo = DEDUP_LO << (bits - 8) if lo is None else int(lo)
    sb = sample_bytes(bits)
    n, out, sa, sb_stride = _pair_operands(payload_a, payload_b, frame_bytes(h, w, siting, bits), "frame_bytes", out, (3, 2))
    hb.check(hb.load().ssm_block_sad_fwd(payload_a.data_ptr(), payload_b.data_ptr(), sa, sb_stride, n, h, w, siting, sb, lo, out.data_ptr(),
                                         hb.stream_ptr()))
    return out


class Repeats:
    """The repeat decision, in Python ints and Fractions and free of the GPU.  blocks: block_counts of the frame.  feed(words) takes the
    six words (max, over of Y, U, V: a row of block_sad / block_sad_host taken with this `lo`) of the next frame n = 1, 2, ... against
    frame n - 1 and returns the frames that this closes, in order: (n, None) for a frame that stays - an ordinary input frame - or
    (n, (r, right, t)) for a repaired repeat: its place is taken by the frame synthesised between frames r and right at the Fraction t.
    The first call also closes frame 0, which is never a repeat.  A frame that is no repeat closes itself and the run before it; a repeat
    waits until its run ends or outgrows dedup_max - so at most dedup_max frames wait.  end() closes the trailing run, every frame of it
    an ordinary one (and frame 0 of a one-frame clip).  `log`: per run (first repeat, m, repaired or not, worst max, worst over) over
    the run's frames and planes."""

    def __init__(self, hi, lo, frac, blocks, dedup_max=DEDUP_MAX):
        self.hi, self.lo, self.frac = int(hi), int(lo), Fraction(frac)
        self.blocks, self.dedup_max = tuple(int(x) for x in blocks), parse_dedup_max(dedup_max)
        assert len(self.blocks) == 3
        self.allowed = tuple((self.frac * x).__floor__() for x in self.blocks)
        self.log = []
        self._fed, self._wait, self._run = 0, [], None          # frames fed; the repeats that wait; the open run as [first, m, max, over]

    def is_repeat(self, words):
        w = [int(x) for x in np.asarray(words).reshape(-1)]
        assert len(w) == 6
        return all(w[2 * p] <= self.hi and w[2 * p + 1] <= self.allowed[p] for p in range(3) if self.blocks[p])

    def _end_run(self, repaired):
        first, m, worst_max, worst_over = self._run
        self.log.append((first, m, repaired, worst_max, worst_over))
        self._run = None

    def feed(self, words):
        self._fed += 1
        n = self._fed
        out = [(0, None)] if n == 1 else []
        w = [int(x) for x in np.asarray(words).reshape(-1)]
        if self.is_repeat(w):
            if self._run is None:
                self._run = [n, 0, 0, 0]
            self._run[1] += 1
            self._run[2], self._run[3] = max(self._run[2], *w[0::2]), max(self._run[3], *w[1::2])
            self._wait.append(n)
            if self._run[1] > self.dedup_max:          # a still: what waited, and every further frame of the run, stays
                out += [(k, None) for k in self._wait]
                self._wait = []
            return out
        if self._run is not None:
            r, g = self._run[0] - 1, self._run[1] + 1
            out += [(k, (r, n, Fraction(k - r, g))) for k in self._wait]
            self._end_run(bool(self._wait))
            self._wait = []
        return out + [(n, None)]

    def end(self):
        out = [(0, None)] if self._fed == 0 else []
        out += [(k, None) for k in self._wait]
        self._wait = []
        if self._run is not None:
            self._end_run(False)
        return out


def dedup_host(frames, h, w, siting=CENTRED, bits=8, dedup=True, dedup_max=DEDUP_MAX):
    """The whole definition in numpy, the yardstick of RepeatSource: payloads [n, frame_bytes] -> (the action of every frame, [(n, None |
    (r, right, t))] as Repeats hands them out, the Repeats that decided, for its log)."""
    frames = np.ascontiguousarray(frames).reshape(-1, frame_bytes(h, w, siting, bits))
    hi, lo, frac = dedup_thresholds(dedup, bits)
    rep, actions = Repeats(hi, lo, frac, block_counts(h, w, siting), dedup_max), []
    if len(frames) > 1:
        for words in block_sad_host(frames[1:], frames[:-1], h, w, siting, bits, lo):
            actions += rep.feed(words)
    actions += rep.end()
    return actions, rep


class RepeatSource(LookAheadSource):
    """A reader that takes the repaired repeats out of a clip: wraps a reader (a TelecineSource for one) and hands out the frames that
    stay, each with the gap before it - `gap` after read_frame_into: 0 for frame 0, 1 after an ordinary neighbour, m + 1 behind a repaired
    run of m repeats - and, a frame ahead, `next_gap`: the gap of the frame that the next call will hand out, 0 at the end of the clip (it
    is what tells a planner whether the pair to the right runs).  on_gap(g), if set, is called once per frame that stays, in order, when
    its gap is known.  It has frames_read (frames handed out), and of the decision so far `repeats` (Repeats.log).

    A chunk is frames_per_chunk new frames behind dedup_max + 1 carried frames on the host and one on the device: ssm_block_sad_fwd takes
    row n + 1 against row n, one stride each.  dedup_max + 1 frames are carried because that many may still be wanted: the repeats that
    wait for the end of their run, and in front of them the frame that stays and waits to be handed out until its right neighbour's gap
    is known.  The repeats' bytes go nowhere; the bytes handed out do not depend on frames_per_chunk."""

    def __init__(self, reader, dev, dedup=True, dedup_max=DEDUP_MAX, frames_per_chunk=8):
        assert frames_per_chunk >= 1
        super().__init__(reader, dev, "the repeat test takes its block differences")
        hi, self.lo, frac = dedup_thresholds(dedup, self.bits)
        self._repeats = Repeats(hi, self.lo, frac, block_counts(self.height, self.width, self.siting), dedup_max)
        self.gap, self.on_gap = None, None
        self._window(frames_per_chunk, self._repeats.dedup_max + 1, 1, [((3, 2), torch.int64)])
        self._last_kept = 0          # _pending: [(a frame that stays, its gap)]

    def _chunk(self):
        """The next chunk: its frames' block differences and what the decision closes."""
        k, c = self._fill(), self._carry
        closed = []
        if k:
            (words,) = self._measure(k, slice(c - 1, c + k), lambda dev, res: block_sad(
                dev[1:], dev[:-1], self.height, self.width, self.siting, self.bits, self.lo, out=res))
            for six in words:
                closed += self._repeats.feed(six)
        if self._eof:
            closed += self._repeats.end()
        for n, act in closed:
            if act is None:          # a frame that stays
                g = n - self._last_kept
                self._pending.append((n, g))
                self._last_kept = n
                if self.on_gap is not None:
                    self.on_gap(g)

    next_gap = property(lambda self: self._pending[0][1] if self._pending else 0)

    def _ahead(self):          # a frame ahead: `next_gap` is known when a frame goes out
        while len(self._pending) < 2 and not self._eof:
            self._chunk()

    def _take(self, kept, out):
        """A frame that stays into `out`; `gap` is then its gap, `next_gap` the next one's."""
        n, self.gap = kept
        assert 0 <= n - self._base < self._np.shape[0], "a frame that stays is among the carried frames or in the chunk"
        out[:] = self._np[n - self._base]

    repeats = property(lambda self: self._repeats.log)


# ---- letterboxed clips: the active area ------------------------------------------------------------------------------------------------
# The definition is in include/ssm_hip.h and DESIGN 3.12: per frame the luma samples above `limit` of every row and column; a line is
# active iff more than FRAC of its samples are; the rectangle is the smallest one that holds every active line of the probed frames,
# aligned outward to the layout's chroma grid.  LIM is the NUMBER of ffmpeg cropdetect's `limit` (24 at 8 bits), not its construction -
# cropdetect averages a line - and FRAC = 1/64 is this module's own: conventions, not backed by a measurement on compressed footage.
ACTIVE_LIMIT, ACTIVE_FRAC = 24, Fraction(1, 64)
ACTIVE_PROBE = 48                  # frames the rectangle is decided on
ACTIVE_MIN = 32                    # a rectangle below this many samples in either direction is no picture: the run goes whole-frame


def active_align(siting):
    """(ay, ax): the rows and columns a rectangle is aligned to in a layout - the luma samples one chroma sample covers."""
    return {CENTRED: (2, 2), COSITED: (2, 2), C422: (1, 2), C444: (1, 1)}[siting]


def active_limit(bits=8, limit=None):
    """The luma code a sample has to exceed to count: `limit` as given, or ACTIVE_LIMIT scaled to the depth."""
    return ACTIVE_LIMIT << (bits - 8) if limit is None else int(limit)


def parse_active(value):
    """The active-area option: None -> None; "auto", "auto:LIM" or "auto:LIM:FRAC" (LIM an integer >= 0 in codes of the clip's depth,
    FRAC a decimal or a fraction in [0, 1)) -> ("auto", LIM or None for the default at the clip's depth, Fraction FRAC); "W:H:X:Y" - the
    order ffmpeg's cropdetect prints, `crop=` in front is fine - or a (w, h, x, y) of whole numbers -> that tuple.  Anything else is a
    ValueError naming the value."""
    if value is None:
        return None
    bad = ValueError("the active area is written auto, auto:LIM, auto:LIM:FRAC or W:H:X:Y (the order of ffmpeg's cropdetect), e.g. auto:24:1/64 "
                     "or 1920:800:0:140 (got %r)" % (value,))
    try:
        if isinstance(value, str):
            parts = value.strip().split(":")
            if parts[0] == "auto":
                if len(parts) > 3:
                    raise bad
                limit = int(parts[1]) if len(parts) > 1 and parts[1] != "" else None
                frac = Fraction(parts[2]) if len(parts) > 2 else ACTIVE_FRAC
                if (limit is not None and not 0 <= limit <= 65535) or not 0 <= frac < 1:
                    raise bad
                return "auto", limit, frac
            if parts[0].startswith("crop="):
                parts[0] = parts[0][5:]
            value = [int(p) for p in parts]
        elif isinstance(value, tuple) and len(value) == 3 and value[0] == "auto":
            return parse_active("auto:%s:%s" % ("" if value[1] is None else value[1], value[2]))
        if len(value) != 4 or any(isinstance(v, bool) or int(v) != v for v in value):
            raise bad
        w, h, x, y = (int(v) for v in value)
    except (ValueError, TypeError, ZeroDivisionError):
        raise bad from None
    if w < 1 or h < 1 or x < 0 or y < 0:
        raise bad
    return w, h, x, y


def parse_active_probe(value):
    """The number of frames the active area is decided on: a whole number of at least 1, or its text."""
    try:
        n = int(value.strip()) if isinstance(value, str) else value
        if isinstance(n, bool) or int(n) != n or n < 1:
            raise ValueError
    except (ValueError, TypeError):
        raise ValueError("active_probe, the frames the active area is decided on, is a whole number of at least 1 (got %r)" % (value,)) from None
    return int(n)


def check_active(rect, h, w, siting):
    """(w', h', x, y) inside an h x w frame of a layout, or the refusal that names the alignment: the origin a multiple of
    active_align(siting), the far edges a multiple of it or the frame's own edge."""
    rw, rh, x, y = rect
    ay, ax = active_align(siting)
    if rw < 1 or rh < 1 or x < 0 or y < 0 or x + rw > w or y + rh > h:
        raise ValueError("the active area %d:%d:%d:%d (W:H:X:Y) lies outside the %dx%d frame (it is aligned to %d columns and %d rows)"
                         % (rw, rh, x, y, w, h, ax, ay))
    if x % ax or y % ay or ((x + rw) % ax and x + rw != w) or ((y + rh) % ay and y + rh != h):
        raise ValueError("the active area %d:%d:%d:%d (W:H:X:Y) is not aligned to %d columns and %d rows, as this chroma layout asks: X and Y "
                         "are multiples of them, X + W and Y + H multiples or the frame's own edge" % (rw, rh, x, y, ax, ay))
    return rw, rh, x, y


def active_counts_host(payload, h, w, bits=8, limit=None):
    """Yardstick of ssm_luma_counts_fwd: payloads [N, at least h * w samples] uint8 (numpy) -> (rows [N, h], cols [N, w]) uint32, the
    number of luma samples of each row and column whose value is above `limit` (None: the default at this depth); a single payload [bytes]
    gives (rows [h], cols [w]).  With bits > 8 over the 16-bit words, all 16 bits.  Chroma is not looked at."""
    payload = np.asarray(payload)
    one = payload.ndim == 1
    above = _luma_of(payload.reshape(1, -1) if one else payload, h, w, bits) > active_limit(bits, limit)
    rows, cols = above.sum(axis=2).astype(np.uint32), above.sum(axis=1).astype(np.uint32)
    return (rows[0], cols[0]) if one else (rows, cols)


class ActiveArea:
    """The decision, in Python ints and Fractions and free of the GPU.  feed(rows, cols) takes one frame's counts (active_counts_host /
    luma_counts) and widens the bounds by the frame's active lines: row r is active iff rows[r] > frac * w, column c iff cols[c] > frac * h,
    exactly.  decide() -> (w', h', x, y): the smallest rectangle that holds every active line fed so far, aligned outward to
    active_align(siting) (origin a multiple, far edges a multiple or the frame's edge) - or None, the whole-frame fallback, with `note`
    saying why: the result is the whole frame, no frame had an active row or column, or it is under ACTIVE_MIN samples in a direction.
    outside(rows, cols, rect) -> (active rows outside the rectangle, active columns outside it) of one frame."""

    def __init__(self, h, w, siting, frac=ACTIVE_FRAC):
        self.h, self.w, self.siting, self.frac = int(h), int(w), siting, Fraction(frac)
        self.bounds, self.fed, self.note = None, 0, None          # [y0, y1, x0, x1), y1 and x1 one past the last active line

    def lines(self, rows, cols):
        """(active rows, active columns) of one frame as bool arrays: count * den > num * length, in Python ints."""
        num, den = self.frac.numerator, self.frac.denominator
        rows, cols = (np.asarray(v).reshape(-1).astype(object) for v in (rows, cols))
        assert rows.size == self.h and cols.size == self.w, "one frame's counts: rows [h] and cols [w]"
        return (rows * den > num * self.w).astype(bool), (cols * den > num * self.h).astype(bool)

    def feed(self, rows, cols):
        self.fed += 1
        ar, ac = (np.flatnonzero(v) for v in self.lines(rows, cols))
        if ar.size == 0 or ac.size == 0:          # a row above the limit puts a sample in some column; a frame with neither has no picture
            return
        b = [int(ar[0]), int(ar[-1]) + 1, int(ac[0]), int(ac[-1]) + 1]
        self.bounds = b if self.bounds is None else [min(self.bounds[0], b[0]), max(self.bounds[1], b[1]), min(self.bounds[2], b[2]),
                                                     max(self.bounds[3], b[3])]

    def decide(self):
        if self.bounds is None:
            self.note = "no active row or column in the %d probed frame%s" % (self.fed, "" if self.fed == 1 else "s")
            return None
        ay, ax = active_align(self.siting)
        y0, y1, x0, x1 = self.bounds
        y0, x0 = y0 - y0 % ay, x0 - x0 % ax
        y1, x1 = min(self.h, -(-y1 // ay) * ay), min(self.w, -(-x1 // ax) * ax)
        rect = (x1 - x0, y1 - y0, x0, y0)
        if rect == (self.w, self.h, 0, 0):
            self.note = "the active area is the whole frame"
            return None
        if rect[0] < ACTIVE_MIN or rect[1] < ACTIVE_MIN:
            self.note = "the active area %d:%d:%d:%d is under %d samples in a direction" % (rect + (ACTIVE_MIN,))
            return None
        self.note = "the active area is %d:%d:%d:%d (W:H:X:Y) of the %dx%d frame, from %d frame%s" % (rect + (self.w, self.h, self.fed,
                                                                                                  "" if self.fed == 1 else "s"))
        return rect

    def outside(self, rows, cols, rect):
        rw, rh, x, y = rect
        ar, ac = self.lines(rows, cols)
        return int(ar[:y].sum() + ar[y + rh:].sum()), int(ac[:x].sum() + ac[x + rw:].sum())


def active_area_host(frames, h, w, siting=CENTRED, bits=8, limit=None, frac=ACTIVE_FRAC, probe=ACTIVE_PROBE):
    """The whole decision in numpy, the yardstick of ActiveSource: payloads [n, frame_bytes] -> ((w', h', x, y) or None, the ActiveArea
    that decided) over the first `probe` frames, or the whole clip if it is shorter."""
    frames = np.ascontiguousarray(frames).reshape(-1, frame_bytes(h, w, siting, bits))
    area = ActiveArea(h, w, siting, frac)
    for rows, cols in zip(*active_counts_host(frames[:probe], h, w, bits, limit)):
        area.feed(rows, cols)
    return area.decide(), area


def _window_slices(h, w, siting, rect):
    """Per plane (Y, U, V) the (row slice, column slice) of a checked rectangle: chroma from y / ay to ceil((y + h') / ay), likewise in x."""
    rw, rh, x, y = check_active(rect, h, w, siting)
    ay, ax = active_align(siting)
    cay, cax = (1, 1) if siting == C444 else ((1, 2) if siting == C422 else (2, 2))          # the chroma subsampling itself
    luma = (slice(y, y + rh), slice(x, x + rw))
    chroma = (slice(y // cay, -(-(y + rh) // cay)), slice(x // cax, -(-(x + rw) // cax)))
    assert (cay, cax) == (ay, ax)
    return luma, chroma, chroma


def cut_window_host(payload, h, w, siting, bits, rect):
    """Yardstick of ssm_window_cut_fwd: payloads [N, frame_bytes(h, w)] uint8 (numpy; a single payload [bytes] gives [bytes]) -> the packed
    payloads of the rectangle (w', h', x, y), [N, frame_bytes(h', w')]: a genuine h' x w' frame of the same layout."""
    payload = np.asarray(payload)
    one = payload.ndim == 1
    src = np.ascontiguousarray(payload).reshape(-1, frame_bytes(h, w, siting, bits))
    out = np.empty((src.shape[0], frame_bytes(rect[1], rect[0], siting, bits)), np.uint8)
    for s, d, (ys, xs) in zip(split_planes(src, h, w, siting, bits), split_planes(out, rect[1], rect[0], siting, bits),
                              _window_slices(h, w, siting, rect)):
        d[...] = s[:, ys, xs]
    return out[0] if one else out


def paste_window_host(window, bars_from, h, w, siting, bits, rect, out=None):
    """The inverse of cut_window_host: a full payload (into `out` if given, which may be bars_from itself) with `window`'s samples inside the
    rectangle and bars_from's bytes outside it, in all three planes.  One payload each, [bytes], or [N, bytes]."""
    window, bars_from = np.asarray(window), np.asarray(bars_from)
    fb = frame_bytes(h, w, siting, bits)
    win = np.ascontiguousarray(window).reshape(-1, frame_bytes(rect[1], rect[0], siting, bits))
    if out is None:
        out = np.empty(bars_from.shape, np.uint8)
    full = out.reshape(-1, fb)          # a view: out is contiguous
    if out is not bars_from:
        full[...] = bars_from.reshape(-1, fb)
    for s, d, (ys, xs) in zip(split_planes(win, rect[1], rect[0], siting, bits), split_planes(full, h, w, siting, bits),
                              _window_slices(h, w, siting, rect)):
        d[:, ys, xs] = s
    return out


def luma_counts(payload, h, w, bits=8, limit=None, rows=None, cols=None):
    """ssm_luma_counts_fwd on payloads: [N, at least h * w samples] uint8 device tensor (unit stride within a row, any row stride) -> (rows
    int32 [N, h], cols int32 [N, w]) on the device (into `rows`, `cols` if given, contiguous): per frame the luma samples of every row and
    column above `limit` (None: the default at this depth).  Whatever the two held before, the call leaves them fully defined."""
    sb = sample_bytes(bits)
    assert payload.is_cuda and payload.dtype == torch.uint8 and payload.dim() == 2 and payload.shape[1] >= h * w * sb and \
        (payload.shape[1] == 1 or payload.stride(1) == 1), "payloads must be a [N, at least h * w samples] uint8 tensor on the GPU with unit stride within a frame"
    n = payload.shape[0]
    rows = torch.empty(n, h, dtype=torch.int32, device=payload.device) if rows is None else rows
    cols = torch.empty(n, w, dtype=torch.int32, device=payload.device) if cols is None else cols
    for t, m in ((rows, h), (cols, w)):
        assert t.is_cuda and t.dtype == torch.int32 and tuple(t.shape) == (n, m) and t.is_contiguous()
    hb.check(hb.load().ssm_luma_counts_fwd(payload.data_ptr(), payload.stride(0) if n > 1 else 0, n, h, w, sb, active_limit(bits, limit),
                                           rows.data_ptr(), cols.data_ptr(), hb.stream_ptr()))
    return rows, cols


def window_cut(frames, h, w, siting, bits, rect, out=None):
    """ssm_window_cut_fwd: [N, at least frame_bytes(h, w)] uint8 device tensor (unit stride within a payload, any row stride) -> the packed
    windows [N, at least frame_bytes(h', w')] of the rectangle (w', h', x, y) (into `out` if given), as cut_window_host."""
    rw, rh, x, y = rect
    n = frames.shape[0]
    si = _field_operand(frames, n, frame_bytes(h, w, siting, bits), "frames")
    wb = frame_bytes(rh, rw, siting, bits) if rw > 0 and rh > 0 else 0
    if out is None:
        out = torch.empty(n, wb, dtype=torch.uint8, device=frames.device)
    so = _field_operand(out, n, wb, "out")
    hb.check(hb.load().ssm_window_cut_fwd(frames.data_ptr(), si, out.data_ptr(), so, n, h, w, y, x, rh, rw, siting, sample_bytes(bits),
                                          hb.stream_ptr()))
    return out


class ActiveSource(LookAheadSource):
    """A reader that finds and watches the active area of a letterboxed clip: wraps a reader (a TelecineSource for one) and hands out its
    frames as they are.  `active`: what parse_active returns - ("auto", limit, frac) or an explicit (w, h, x, y), checked against the
    frame.  decide() -> `area`, the rectangle or None for a whole-frame run, and `note`, one line that says which and why; with "auto" it
    reads the first `probe` frames (or the whole clip if it is shorter), counts them on the GPU, decides (ActiveArea) and replays them.
    With an area, every later frame is counted a chunk ahead of the loop, and a frame with active rows or columns outside the rectangle
    goes to `excess` as (frame index, rows outside, columns outside); it changes nothing else.  Without one (the fallback) the frames
    behind the probe come straight from the reader.

    A chunk is frames_per_chunk frames, none carried, for one ssm_luma_counts_fwd; its buffers are made when the first frame is counted,
    so a whole-frame run with an explicit rectangle makes none.  The bytes handed out do not depend on frames_per_chunk or probe."""

    def __init__(self, reader, dev, active=("auto", None, ACTIVE_FRAC), probe=ACTIVE_PROBE, frames_per_chunk=8):
        assert frames_per_chunk >= 1
        super().__init__(reader, dev, "the active area takes its luma counts")
        active = parse_active(active)
        assert active is not None
        self.auto = active[0] == "auto"
        self.limit = active_limit(self.bits, active[1] if self.auto else None)
        self._area = ActiveArea(self.height, self.width, self.siting, active[2] if self.auto else ACTIVE_FRAC)
        self._given = None if self.auto else check_active(active, self.height, self.width, self.siting)
        self.probe, self.area, self.note, self.excess = parse_active_probe(probe), None, None, []
        self._rows, self._decided, self._counted = frames_per_chunk, False, 0          # _counted: the clip's frames counted so far

    def _count(self, k):
        """The counts of the first k rows of the pinned buffer: (rows [k, h], cols [k, w]) uint32, views of pinned memory."""
        return self._measure(k, slice(0, k), lambda dev, rows, cols: luma_counts(dev, self.height, self.width, self.bits, self.limit, rows, cols))

    def _buffers(self):
        if self._np is None:
            self._window(self._rows, 0, 0, [((self.height,), torch.int32), ((self.width,), torch.int32)])

    def decide(self):
        """The rectangle of the run, (w, h, x, y), or None: a whole-frame run; `note` says why.  Reads the probe frames on the first call."""
        if self._decided:
            return self.area
        self._decided = True
        if self.auto:
            self._buffers()
            probe = self._probe(self.probe)
            for at in range(0, len(probe), self._rows):
                k = min(self._rows, len(probe) - at)
                self._np[:k] = probe[at:at + k]
                for r, c in zip(*self._count(k)):
                    self._area.feed(r, c)
            self.area, self.note = self._area.decide(), self._area.note
            self._counted = len(probe)          # inside the rectangle by construction
        else:
            whole = self._given == (self.width, self.height, 0, 0)
            self.area = None if whole else self._given
            self.note = "the active area is the whole frame" if whole else "the active area is %d:%d:%d:%d (W:H:X:Y), as given" % self._given
        self._straight = self.area is None
        return self.area

    def _chunk(self):
        """The next chunk behind the probe: its frames' counts, and the frames that leave the rectangle to `excess`."""
        self._buffers()
        k = self._fill()
        if k:
            for r, c in zip(*self._count(k)):
                out = self._area.outside(r, c, self.area)
                if out != (0, 0):
                    self.excess.append((self._counted,) + out)
                self._counted += 1
            self._pending = list(range(self._base, self._base + k))

    def _ahead(self):
        if self.decide() is not None and not self._replay:
            while not self._pending and not self._eof:
                self._chunk()


# ---- blocks that do not change ---------------------------------------------------------------------------------------------------------
# The definition is in include/ssm_hip.h and DESIGN 3.12: block (bx, by) of a frame is its 8 x 8 luma samples at (8 bx, 8 by) with the U and
# V samples under them; it is static in a pair iff the sum of |a - b| over all of them is at most `lo`, and every frame between the two
# then carries the left frame's samples of the block.  lo = 0 - the two frames agree - is exact; any other lo is the user's number.
STATIC_MAX = (1 << 24) - 1         # the largest `lo` ssm_static_paste_fwd takes: above every block sum (192 * 65535)


def parse_static(text):
    """The threshold of the static-block test, a whole number in 0 .. 2^24 - 1 in codes of the clip's depth (0: the block is the same in
    both frames), as an int or a command line's text -> int.  Anything else is a ValueError naming the value."""
    try:
        if isinstance(text, bool) or (not isinstance(text, str) and int(text) != text):
            raise ValueError
        lo = int(text.strip() if isinstance(text, str) else text)
    except (ValueError, TypeError, OverflowError):
        raise ValueError("static, the largest block sum of |difference| that counts as unchanged, is a whole number in 0 .. 2^24 - 1 "
                         "(got %r)" % (text,)) from None
    if not 0 <= lo <= STATIC_MAX:
        raise ValueError("static, the largest block sum of |difference| that counts as unchanged, is a whole number in 0 .. 2^24 - 1 "
                         "(got %r)" % (text,))
    return lo


def static_blocks(h, w):
    """The 8 x 8 blocks of an h x w frame: (h >> 3) * (w >> 3), 0 for a frame below 8 rows or columns."""
    return (h >> 3) * (w >> 3)


def _chroma_block(siting):
    """(rows, columns) of the chroma samples under an 8 x 8 luma block."""
    return (8, 8) if siting == C444 else (8, 4) if siting == C422 else (4, 4)


def static_paste_host(outputs, a, b, h, w, siting, bits=8, lo=0):
    """Yardstick of ssm_static_paste_fwd: outputs [N, T, at least frame_bytes] uint8 (numpy), the T frames between the payloads a[n] and
    b[n] ([N, at least frame_bytes] uint8) -> (a copy of `outputs` in which the samples of every block that is static in pair n - the sum
    of |a - b| over its luma, U and V samples at most `lo` - are a[n]'s, uint64 [N]: the static blocks of every pair).  With bits > 8
    over the 16-bit words, all 16 bits."""
    lo, fb = int(lo), frame_bytes(h, w, siting, bits)
    outputs, a, b = (np.asarray(x) for x in (outputs, a, b))
    assert outputs.dtype == np.uint8 and outputs.ndim == 3 and outputs.shape[2] >= fb, "outputs are [N, T, at least frame_bytes] uint8"
    n, t = outputs.shape[:2]
    for p in (a, b):
        assert p.dtype == np.uint8 and p.shape == (n, p.shape[1]) and p.shape[1] >= fb, "payloads are [N, at least frame_bytes] uint8"
    res, counts = outputs.copy(), np.zeros(n, np.uint64)
    by, bx = h >> 3, w >> 3
    if not (by and bx and n and t):
        return res, counts
    pa, pb = (split_planes(np.ascontiguousarray(x[:, :fb]), h, w, siting, bits) for x in (a, b))
    cr, cc = _chroma_block(siting)
    shapes = ((8, 8), (cr, cc), (cr, cc))
    d = np.zeros((n, by, bx), np.int64)
    for (x, y), (rr, rc) in zip(zip(pa, pb), shapes):
        diff = np.abs(x[:, :rr * by, :rc * bx].astype(np.int64) - y[:, :rr * by, :rc * bx].astype(np.int64))
        d += diff.reshape(n, by, rr, bx, rc).sum(axis=(2, 4))
    keep = d <= lo                                   # [N, by, bx]
    counts[:] = keep.reshape(n, -1).sum(axis=1)
    frames = np.ascontiguousarray(res[:, :, :fb]).reshape(n * t, fb)
    for plane, src, (rr, rc) in zip(split_planes(frames, h, w, siting, bits), pa, shapes):
        mask = np.repeat(np.repeat(keep, rr, axis=1), rc, axis=2)          # [N, rr by, rc bx]
        dst = plane.reshape((n, t) + plane.shape[1:])[:, :, :rr * by, :rc * bx]
        np.copyto(dst, src[:, None, :rr * by, :rc * bx], where=mask[:, None])
    res[:, :, :fb] = frames.reshape(n, t, fb)
    return res, counts


def static_paste(payload_a, payload_b, outputs, h, w, siting, bits=8, lo=0, counts=None):
    """ssm_static_paste_fwd on payloads: a, b [N, at least frame_bytes] uint8 device tensors (unit stride within a row, any row stride:
    frames n and n + 1 of one buffer are fine) and outputs [N * T, at least frame_bytes], the T frames of pair n in rows n T .. n T + T - 1,
    changed in place: the samples of every block that is static in pair n become a[n]'s.  -> int64 [N] on the device (into `counts` if
    given): the static blocks of every pair.  Queued on the current stream."""
    fb = frame_bytes(h, w, siting, bits)
    n, counts, sa, sb_stride = _pair_operands(payload_a, payload_b, fb, "frame_bytes", counts, ())
    assert outputs.is_cuda and outputs.dtype == torch.uint8 and outputs.dim() == 2 and outputs.shape[1] >= fb and outputs.device == payload_a.device \
        and (outputs.shape[1] == 1 or outputs.stride(1) == 1), "outputs must be [N * T, at least frame_bytes] uint8 on the payloads' device"
    assert outputs.shape[0] >= n and outputs.shape[0] % n == 0, "outputs hold T rows per pair"
    t = outputs.shape[0] // n
    hb.check(hb.load().ssm_static_paste_fwd(payload_a.data_ptr(), payload_b.data_ptr(), sa, sb_stride, outputs.data_ptr(),
                                            outputs.stride(0) if n * t > 1 else 0, n, t, h, w, siting, sample_bytes(bits), int(lo),
                                            counts.data_ptr(), hb.stream_ptr()))
    return counts


# ---- the flow check's per-block fallback -------------------------------------------------------------------------------------------------
# The definition is in include/ssm_hip.h and DESIGN 3.12: the blocks are static_blocks'; a block fails in a pair iff more than K of its 64
# luma positions are inconsistent in at least one direction of the pair's mask (ssm_flow_consistency_fwd), and an output between the two
# frames then carries the NEARER frame's samples of the block.  K has no default.
FLOW_BLOCKS_MAX = 64               # a block has 64 luma positions: K = 64 fails nothing


def parse_flow_blocks(value, spelt="flow_blocks"):
    """The K of the per-block fallback, a whole number in 0 .. 64, as an int or a command line's text -> int.  Anything else is a
    ValueError naming the value."""
    text = "%s, the most inconsistent pixels of an 8 x 8 block that still passes, is a whole number in 0 .. 64 (got %r)" % (spelt, value)
    try:
        if isinstance(value, bool) or (not isinstance(value, str) and int(value) != value):
            raise ValueError
        k = int(value.strip() if isinstance(value, str) else value)
    except (ValueError, TypeError, OverflowError):
        raise ValueError(text) from None
    if not 0 <= k <= FLOW_BLOCKS_MAX:
        raise ValueError(text)
    return k


def fixed_split(rate):
    """Of the upsample_rate - 1 outputs of a pair on the fixed grid, t = (j + 1) / rate, the number below 1/2: they take the left frame."""
    return sum(1 for j in range(rate - 1) if 2 * (j + 1) < rate)


def times_split(times):
    """The same for a pair's exact times (Fractions, ascending - asserted: the outputs below 1/2 are then the first rows)."""
    times = list(times)
    assert all(x < y for x, y in zip(times, times[1:])), "a pair's times ascend in its output rows"
    return sum(1 for t in times if t < Fraction(1, 2))


def flow_block_counts_host(mask, h, w):
    """n of every block: mask [N, 2, h, w] uint8 -> int64 [N, h >> 3, w >> 3], the luma positions with bit 0 of mask[0] | mask[1] set."""
    mask = np.asarray(mask)
    assert mask.dtype == np.uint8 and mask.ndim == 4 and mask.shape[1:] == (2, h, w), "mask is [N, 2, h, w] uint8"
    by, bx = h >> 3, w >> 3
    bad = ((mask[:, 0] | mask[:, 1]) & 1)[:, :8 * by, :8 * bx].astype(np.int64)
    return bad.reshape(mask.shape[0], by, 8, bx, 8).sum(axis=(2, 4))


def flow_paste_host(outputs, a, b, mask, h, w, siting, bits=8, k=FLOW_BLOCKS_MAX, split=0):
    """Yardstick of ssm_flow_paste_fwd: outputs [N, T, at least frame_bytes] uint8 (numpy), the T frames between the payloads a[n] and
    b[n] ([N, at least frame_bytes] uint8), mask [N, 2, h, w] uint8 as flow_consistency_host writes it -> (a copy of `outputs` in which
    the samples of every block that fails in pair n - more than k of its 64 luma positions have bit 0 of mask[n, 0] | mask[n, 1] set -
    are a[n]'s in the outputs j < split and b[n]'s in the outputs j >= split, uint64 [N]: the failed blocks of every pair)."""
    k, split, fb = int(k), int(split), frame_bytes(h, w, siting, bits)
    outputs, a, b = (np.asarray(x) for x in (outputs, a, b))
    assert outputs.dtype == np.uint8 and outputs.ndim == 3 and outputs.shape[2] >= fb, "outputs are [N, T, at least frame_bytes] uint8"
    n, t = outputs.shape[:2]
    assert 0 <= k <= FLOW_BLOCKS_MAX and 0 <= split <= t, "k in 0 .. 64, split in 0 .. T"
    for p in (a, b):
        assert p.dtype == np.uint8 and p.shape == (n, p.shape[1]) and p.shape[1] >= fb, "payloads are [N, at least frame_bytes] uint8"
    res, counts = outputs.copy(), np.zeros(n, np.uint64)
    by, bx = h >> 3, w >> 3
    if not (by and bx and n and t):
        return res, counts
    fail = flow_block_counts_host(np.asarray(mask)[:n], h, w) > k          # [N, by, bx]
    counts[:] = fail.reshape(n, -1).sum(axis=1)
    pa, pb = (split_planes(np.ascontiguousarray(x[:, :fb]), h, w, siting, bits) for x in (a, b))
    cr, cc = _chroma_block(siting)
    frames = np.ascontiguousarray(res[:, :, :fb]).reshape(n * t, fb)
    for plane, sa, sb, (rr, rc) in zip(split_planes(frames, h, w, siting, bits), pa, pb, ((8, 8), (cr, cc), (cr, cc))):
        where = np.repeat(np.repeat(fail, rr, axis=1), rc, axis=2)[:, None]          # [N, 1, rr by, rc bx]
        dst = plane.reshape((n, t) + plane.shape[1:])[:, :, :rr * by, :rc * bx]
        np.copyto(dst[:, :split], sa[:, None, :rr * by, :rc * bx], where=where)
        np.copyto(dst[:, split:], sb[:, None, :rr * by, :rc * bx], where=where)
    res[:, :, :fb] = frames.reshape(n, t, fb)
    return res, counts


def flow_paste(payload_a, payload_b, outputs, mask, h, w, siting, bits, k, split, counts=None):
    """ssm_flow_paste_fwd on payloads: a, b [N, at least frame_bytes] uint8 device tensors (unit stride within a row, any row stride:
    frames n and n + 1 of one buffer are fine), outputs [N * T, at least frame_bytes], the T frames of pair n in rows n T .. n T + T - 1,
    changed in place, and mask, uint8 [N, 2, h, w] on the device with dense planes (flow_consistency(..., want_mask=True)): the samples
    of every block that fails in pair n become a[n]'s in its outputs j < split and b[n]'s from there on.  -> int64 [N] on the device (into
    `counts` if given): the failed blocks of every pair.  Queued on the current stream."""
    fb = frame_bytes(h, w, siting, bits)
    n, counts, sa, sb_stride = _pair_operands(payload_a, payload_b, fb, "frame_bytes", counts, ())
    assert outputs.is_cuda and outputs.dtype == torch.uint8 and outputs.dim() == 2 and outputs.shape[1] >= fb and outputs.device == payload_a.device \
        and (outputs.shape[1] == 1 or outputs.stride(1) == 1), "outputs must be [N * T, at least frame_bytes] uint8 on the payloads' device"
    assert outputs.shape[0] >= n and outputs.shape[0] % n == 0, "outputs hold T rows per pair"
    assert mask.is_cuda and mask.dtype == torch.uint8 and tuple(mask.shape) == (n, 2, h, w) and mask.device == payload_a.device \
        and mask[0].is_contiguous(), "mask must be [N, 2, h, w] uint8 on the payloads' device, a pair's two planes dense"
    t = outputs.shape[0] // n
    hb.check(hb.load().ssm_flow_paste_fwd(payload_a.data_ptr(), payload_b.data_ptr(), sa, sb_stride, outputs.data_ptr(),
                                          outputs.stride(0) if n * t > 1 else 0, n, t, int(split), h, w, siting, sample_bytes(bits),
                                          mask.data_ptr(), mask.stride(0) if n > 1 else 0, int(k), counts.data_ptr(), hb.stream_ptr()))
    return counts


# The fallback of a failed block: "nearer" is the rule above; "mix" is the cross-fade a (1 - t) + b t of the pair's two frames at the
# output's exact time, rounded half up (include/ssm_hip.h, ssm_flow_mix_fwd).  The times of a pair's outputs reach the kernel as
# k_j / den with k_j = num0 + j num_step, three launch scalars; den is at most FLOW_MIX_DEN_MAX (the numerator then fits 32 bits).
FLOW_FALLBACKS = ("nearer", "mix")
FLOW_MIX_DEN_MAX = 65535


def parse_flow_fallback(value, spelt="flow_fallback"):
    """What a failed block of the per-block fallback carries, "nearer" or "mix".  Anything else is a ValueError naming the value."""
    name = value.strip().lower() if isinstance(value, str) else value
    if name not in FLOW_FALLBACKS:
        raise ValueError("%s, what a failed block of the per-block fallback carries, is \"nearer\" (the nearer input frame's samples) or "
                         "\"mix\" (the cross-fade of the two frames at the output's time) (got %r)" % (spelt, value))
    return name


def flow_mix_den(tl):
    """The den of ssm_flow_mix_fwd for a clip on the Timeline `tl`: the denominator of its step, which every output's t = frac(k step)
    is a multiple of.  A denominator above FLOW_MIX_DEN_MAX is a ValueError that names it and the limit."""
    den = tl.step.denominator
    if den > FLOW_MIX_DEN_MAX:
        raise ValueError("flow_fallback=\"mix\" takes the outputs' times as whole numbers over the denominator of the timeline's step, and the "
                         "step %s has the denominator %d, more than %d: round the rate or the speed, or use the fallback \"nearer\""
                         % (tl.step, den, FLOW_MIX_DEN_MAX))
    return den


def fixed_mix(rate):
    """(num0, num_step, den) of the upsample_rate - 1 outputs of a pair on the fixed grid, t = (j + 1) / rate."""
    return 1, 1, int(rate)


def times_mix(times, den):
    """The same for a pair's exact times (Fractions over `den`, an arithmetic progression - asserted: the kernel makes them of three
    scalars); one output has the step 0.  den = 1 (an integer step) has no synthesised frame and no times."""
    ks = [t * den for t in times]
    assert ks and all(k.denominator == 1 and 0 <= k <= den for k in ks), "a pair's times are whole numbers over den, in 0 .. 1"
    num0, num_step = int(ks[0]), int(ks[1] - ks[0]) if len(ks) > 1 else 0
    assert all(k == num0 + j * num_step for j, k in enumerate(ks)), "a pair's times step evenly in its output rows"
    return num0, num_step, int(den)


def flow_mix_host(outputs, a, b, mask, h, w, siting, bits=8, k=FLOW_BLOCKS_MAX, num0=1, num_step=1, den=2):
    """Yardstick of ssm_flow_mix_fwd: the operands of flow_paste_host -> (a copy of `outputs` in which every sample of every block that
    fails in pair n - flow_paste_host's blocks and test, by flow_block_counts_host - is, in output j,
    (a (den - k_j) + b k_j + (den >> 1)) // den with k_j = num0 + j num_step, over the samples of a[n] and b[n] (bytes, or the 16-bit
    words above 8 bits) in int64 with numpy's floor division, uint64 [N]: the failed blocks of every pair)."""
    k, num0, num_step, den, fb = int(k), int(num0), int(num_step), int(den), frame_bytes(h, w, siting, bits)
    outputs, a, b = (np.asarray(x) for x in (outputs, a, b))
    assert outputs.dtype == np.uint8 and outputs.ndim == 3 and outputs.shape[2] >= fb, "outputs are [N, T, at least frame_bytes] uint8"
    n, t = outputs.shape[:2]
    ks = [num0 + j * num_step for j in range(t)]
    assert 0 <= k <= FLOW_BLOCKS_MAX and 2 <= den <= FLOW_MIX_DEN_MAX and all(0 <= kj <= den for kj in ks), \
        "k in 0 .. 64, den in 2 .. 65535, every num0 + j num_step in 0 .. den"
    for p in (a, b):
        assert p.dtype == np.uint8 and p.shape == (n, p.shape[1]) and p.shape[1] >= fb, "payloads are [N, at least frame_bytes] uint8"
    res, counts = outputs.copy(), np.zeros(n, np.uint64)
    by, bx = h >> 3, w >> 3
    if not (by and bx and n and t):
        return res, counts
    fail = flow_block_counts_host(np.asarray(mask)[:n], h, w) > k          # [N, by, bx]
    counts[:] = fail.reshape(n, -1).sum(axis=1)
    pa, pb = (split_planes(np.ascontiguousarray(x[:, :fb]), h, w, siting, bits) for x in (a, b))
    cr, cc = _chroma_block(siting)
    frames = np.ascontiguousarray(res[:, :, :fb]).reshape(n * t, fb)
    for plane, sa, sb, (rr, rc) in zip(split_planes(frames, h, w, siting, bits), pa, pb, ((8, 8), (cr, cc), (cr, cc))):
        where = np.repeat(np.repeat(fail, rr, axis=1), rc, axis=2)          # [N, rr by, rc bx]
        dst = plane.reshape((n, t) + plane.shape[1:])[:, :, :rr * by, :rc * bx]
        xa, xb = (s[:, :rr * by, :rc * bx].astype(np.int64) for s in (sa, sb))
        for j, kj in enumerate(ks):
            np.copyto(dst[:, j], ((xa * (den - kj) + xb * kj + (den >> 1)) // den).astype(plane.dtype), where=where)
    res[:, :, :fb] = frames.reshape(n, t, fb)
    return res, counts


def flow_mix(payload_a, payload_b, outputs, mask, h, w, siting, bits, k, num0, num_step, den, counts=None):
    """ssm_flow_mix_fwd on payloads: the operands of flow_paste; the samples of every block that fails in pair n become, in its output j,
    the cross-fade of a[n]'s and b[n]'s at k_j / den, k_j = num0 + j num_step, rounded half up (flow_mix_host).  -> int64 [N] on the
    device (into `counts` if given): the failed blocks of every pair.  Queued on the current stream."""
    fb = frame_bytes(h, w, siting, bits)
    n, counts, sa, sb_stride = _pair_operands(payload_a, payload_b, fb, "frame_bytes", counts, ())
    assert outputs.is_cuda and outputs.dtype == torch.uint8 and outputs.dim() == 2 and outputs.shape[1] >= fb and outputs.device == payload_a.device \
        and (outputs.shape[1] == 1 or outputs.stride(1) == 1), "outputs must be [N * T, at least frame_bytes] uint8 on the payloads' device"
    assert outputs.shape[0] >= n and outputs.shape[0] % n == 0, "outputs hold T rows per pair"
    assert mask.is_cuda and mask.dtype == torch.uint8 and tuple(mask.shape) == (n, 2, h, w) and mask.device == payload_a.device \
        and mask[0].is_contiguous(), "mask must be [N, 2, h, w] uint8 on the payloads' device, a pair's two planes dense"
    t = outputs.shape[0] // n
    hb.check(hb.load().ssm_flow_mix_fwd(payload_a.data_ptr(), payload_b.data_ptr(), sa, sb_stride, outputs.data_ptr(),
                                        outputs.stride(0) if n * t > 1 else 0, n, t, int(num0), int(num_step), int(den), h, w, siting,
                                        sample_bytes(bits), mask.data_ptr(), mask.stride(0) if n > 1 else 0, int(k), counts.data_ptr(),
                                        hb.stream_ptr()))
    return counts


# ---- output order -------------------------------------------------------------------------------------------------------------------
def pass_order(valid, nt):
    """Write order of one pass of `valid` pairs with nt interpolated frames each: ("interp", row of the pass's output buffer) for the
    frames between a pair, then ("orig", row of the pass's input buffer) for the pair's right frame, its own input bytes."""
    for p in range(valid):
        for i in range(nt):
            yield "interp", p * nt + i
        yield "orig", p


def clip_order(n_frames, rate, pairs_per_batch=1):
    """The output of an n-frame clip as (input frame index, step): step 0 is input frame `index` itself, step s in 1..rate-1 the frame
    at t = s / rate between inputs `index` and `index + 1`.  (n - 1) * rate + 1 entries; composed of pass_order as run() composes it."""
    out = [(0, 0)] if n_frames > 0 else []
    nt, done = rate - 1, 0
    while done < n_frames - 1:
        valid = min(pairs_per_batch, n_frames - 1 - done)
        for kind, row in pass_order(valid, nt):
            out.append((done + row // nt, row % nt + 1) if kind == "interp" else (done + row + 1, 0))
        done += valid
    return out


def output_rate(rate, upsample_rate, slowmo=False):
    """Frame rate (num, den) of the output header: the input's times upsample_rate (same duration), or with slowmo the input's."""
    return (rate[0], rate[1]) if slowmo else (rate[0] * int(upsample_rate), rate[1])


# ---- the output timeline: any frame rate, any speed ----------------------------------------------------------------------------------
# The stage-2 batch of a pass is pairs_per_batch * slots.  The widest tensor of the decoder (up-sampled 512 channels beside a 512-channel
# skip) goes through its element-wise kernels in groups of 4 channels on the grid's z axis together with the batch: 256 groups * batch
# has to stay within 65535, so a plan takes at most 255 stage-2 entries - the largest upsample_rate - 1 at one pair per pass.
MAX_STAGE2_BATCH = 255
MAX_PERIOD = 1 << 20          # min(numerator, denominator) of a step: the pattern's period, walked once to find `slots`


def parse_rate(text):
    """"60", "60:1" or "60000:1001" -> (num, den), as written (not reduced); anything else is a ValueError naming the text."""
    m = re.fullmatch(r"(\d+)(?::(\d+))?", str(text).strip())
    if not m or int(m.group(1)) < 1 or (m.group(2) is not None and int(m.group(2)) < 1):
        raise ValueError("a frame rate is written N or N:D with positive integers, e.g. 60 or 60000:1001 (got %r)" % (text,))
    return int(m.group(1)), int(m.group(2) or 1)


def parse_speed(text):
    """"0.25", "1/4" or "3/10" (or a number, or a Fraction) -> Fraction > 0; anything else is a ValueError naming the value."""
    try:
        s = Fraction(text.strip() if isinstance(text, str) else text)
    except (ValueError, TypeError, ZeroDivisionError):
        raise ValueError("a speed is written as a decimal or a fraction, e.g. 0.25, 1/4 or 3/10 (got %r)" % (text,)) from None
    if s <= 0:
        raise ValueError("a speed must be positive (got %r)" % (text,))
    return s


def parse_shutter(text):
    """A shutter angle in degrees, "180", "172.8" or "90" (or a number, or a Fraction) -> the open fraction angle / 360 as an exact
    Fraction in (0, 1]; anything else is a ValueError naming the value."""
    try:
        deg = Fraction(text.strip() if isinstance(text, str) else text)
    except (ValueError, TypeError, ZeroDivisionError):
        raise ValueError("a shutter angle is written in degrees as a decimal or a fraction, e.g. 180, 172.8 or 90 (got %r)" % (text,)) from None
    if not 0 < deg <= 360:
        raise ValueError("a shutter angle lies above 0 and at most at 360 degrees (got %r)" % (text,))
    return deg / 360


# Shutter windows: the weights of an output's S sub-frames.  Sample j sits at u_j = (j + 1/2) / S of the open interval - symmetric in j, so
# the blur's centre of mass stays where the box puts it.  "box" is no weighted call at all: the loop as it was before there were windows.
SHUTTER_WINDOWS = ("box", "triangle", "hann", "gauss")
GAUSS_K = Fraction(2)          # gauss spans +-K standard deviations over the open interval; 2 is a convention, not a measured optimum
ACC_WEIGHTS_MAX = hb.SSM_ACC_WEIGHTS_MAX


def parse_shutter_window(text):
    """"box", "triangle", "hann", "gauss" or "gauss:K" with K a positive decimal or fraction ("gauss" is "gauss:2") -> (name, K or None);
    anything else is a ValueError naming the value."""
    names = "box, triangle, hann, gauss[:K]"
    if isinstance(text, tuple) and len(text) == 2 and text[0] in SHUTTER_WINDOWS:
        text = text[0] if text[1] is None else "%s:%s" % text
    if not isinstance(text, str):
        raise ValueError("unknown shutter_window %r: it is one of %s" % (text, names))
    name, colon, arg = text.strip().partition(":")
    if name not in SHUTTER_WINDOWS or (colon and name != "gauss"):
        raise ValueError("unknown shutter_window %r: it is one of %s" % (text, names))
    if name != "gauss":
        return name, None
    if not colon:
        return name, GAUSS_K
    try:
        k = Fraction(arg.strip())
    except (ValueError, ZeroDivisionError):
        raise ValueError("shutter_window %r: K of gauss:K is written as a decimal or a fraction, e.g. 2, 2.5 or 5/2" % (text,)) from None
    if k <= 0:
        raise ValueError("shutter_window %r: K of gauss:K must be positive" % (text,))
    return name, k


def window_name(window):
    """A parsed window as it is written: "hann", "gauss:2", "gauss:5/2"."""
    name, k = parse_shutter_window(window)
    return name if k is None else "%s:%s" % (name, k)


def shutter_window(name, S):
    """(w, scale) of a shutter window over S samples: w the S float32 weights, scale = float32(1 / sum of float64(w_j)) - the sum of the
    fp32 weights taken in float64, one division, rounded once.  With u_j = (j + 1/2) / S:
      box        w_j = 1: what the unweighted calls compute, here for the record - the streamed loop makes no weighted call for it
      triangle   w_j = min(2 j + 1, 2 (S - j) - 1): odd integers, exact in fp32, proportional to 1 - |2 u_j - 1|
      hann       w_j = float32(sin^2(pi u_j)), evaluated in float64
      gauss[:K]  w_j = float32(exp(-1/2 (K (2 u_j - 1))^2)), evaluated in float64: the window spans +-K standard deviations (default 2)
    `name` is what parse_shutter_window takes or returns."""
    name, k = parse_shutter_window(name)
    if isinstance(S, bool) or int(S) != S or S < 1:
        raise ValueError("a shutter window has at least 1 sample (got %r)" % (S,))
    S = int(S)
    j = np.arange(S, dtype=np.float64)
    u = (j + 0.5) / S
    if name == "box":
        w = np.ones(S)
    elif name == "triangle":
        w = np.minimum(2 * j + 1, 2 * (S - j) - 1)
    elif name == "hann":
        w = np.sin(np.pi * u) ** 2
    else:
        w = np.exp(-0.5 * (float(k) * (2.0 * u - 1.0)) ** 2)
    w = w.astype(_F)
    return w, _F(1.0 / w.astype(np.float64).sum())


def parse_scene_cut(text):
    """A scene-cut threshold, "0.1" or "1/10" (or a number, or a Fraction) -> Fraction in (0, 1]; anything else is a ValueError naming
    the value."""
    try:
        th = Fraction(text.strip() if isinstance(text, str) else text)
    except (ValueError, TypeError, ZeroDivisionError):
        raise ValueError("a scene-cut threshold is written as a decimal or a fraction, e.g. 0.1 or 1/10 (got %r)" % (text,)) from None
    if not 0 < th <= 1:
        raise ValueError("a scene-cut threshold lies above 0 and at most at 1 (got %r)" % (text,))
    return th


class SceneCuts:
    """Which pairs of input frames are scene cuts, from their luma sums (luma_sad / luma_sad_host); no GPU in it, every quantity an
    integer or a Fraction.  feed(s, pixels) takes the pairs in the order in which they run - a pair that a timeline skips is not fed -
    and returns (is a cut, score):
        m = Fraction(s, pixels)                      the mean absolute luma difference of the pair, 0 .. 255
        score = min(m, |m - m_prev|) / 255           m_prev: the m of the pair fed before, 0 before the first
        a cut iff score >= threshold                 then m_prev = m
    The mean absolute frame difference damped by its own change: steady fast motion has a large m that changes little, a cut is a spike.
    The first pair has nothing to be compared with and scores its m.  This is a convention and NOT backed by a measurement here; the
    threshold, a Fraction in (0, 1], has no default and is the user's to choose.  Fades and dissolves are not looked for."""

    def __init__(self, threshold):
        self.threshold = parse_scene_cut(threshold)
        self.m_prev = Fraction(0)

    def feed(self, s, pixels):
        m = Fraction(int(s), int(pixels))
        score = min(m, abs(m - self.m_prev)) / 255
        self.m_prev = m
        return score >= self.threshold, score


def timeline_step(in_rate, target_rate=None, speed=None):
    """step = speed * in_rate / out_rate as a Fraction: how far the input clock moves per output frame.  target_rate None: the input's
    rate; speed None: 1."""
    in_rate = Fraction(int(in_rate[0]), int(in_rate[1]))
    out_rate = in_rate if target_rate is None else Fraction(int(target_rate[0]), int(target_rate[1]))
    return (Fraction(1) if speed is None else parse_speed(speed)) * in_rate / out_rate


class Timeline:
    """Where every output frame sits on the input's clock.  Input frame i sits at time i; output frame k at tau_k = k * step, for
    k = 0 .. floor((n - 1) / step) of an n-frame clip.  With i = floor(tau_k) and t = tau_k - i: t == 0 is input frame i's own bytes,
    anything else the frame synthesised between inputs i and i + 1 at t.  All of it in Fractions and in closed form from k - no time is
    ever accumulated, so a long clip drifts by nothing.

    The engine's time is t32(t) = np.float32(t.numerator / t.denominator): the exact ratio rounded once to float64 by the division and
    once more to float32 - the rule of evaluation.t_values (idx / float(rate), then the tensor's float32), so step = 1/R gives its times
    bit for bit.

    slots: the most synthesised frames any one pair gets - the engine's times per pair.  step = a/b in lowest terms repeats every b
    outputs (a inputs), so one period decides it.  A speed that changes within a clip would replace `step` by a function of k here.

    The shutter (include/ssm_hip.h spells the definition): shutter = sigma in (0, 1], the open fraction of the output interval, and
    samples = S.  Output frame k is the mean of S sub-frames at tau(k, j) = k step + j d, d = sigma step / S, j = 0 .. S - 1, and exists
    iff its last one does: tau(k, S - 1) <= n - 1.  With sigma = p/q in lowest terms every sample sits on the uniform grid g = step / (q S):
    tau(k, j) = (k q S + j p) g, and because (S - 1) p < q S the samples of output k all come before those of output k + 1 - the samples
    in time order are the (k, j) in lexicographic order, sample number r is (k, j) = divmod(r, S).  The closed forms below count grid
    points, with or without a shutter: at S = 1 the grid is g = step / q and tau(k, 0) = k q g = k step, the timeline above whatever the
    shutter.  Only the shape of what comes back differs.  With S > 1
      outputs(n), feed()   deliver one tuple of S (i, t) per output frame instead of one (i, t)
      times(i)             [(t, k, j)]: each synthesised sample with the output and the place in it that it belongs to
      on_frame(i)          the (k, j) of the sample that is input frame i itself, or None
      slots                the most synthesised SAMPLES any one pair gets."""

    def __init__(self, step, max_slots=None, shutter=None, samples=1):
        try:
            step = Fraction(step)
        except (ValueError, TypeError, ZeroDivisionError):
            raise ValueError("the timeline's step must be a number or a fraction (got %r)" % (step,)) from None
        if step <= 0:
            raise ValueError("the timeline's step (speed * input rate / output rate) must be positive (got %s)" % step)
        self.step, self.a, self.b = step, step.numerator, step.denominator
        if min(self.a, self.b) > MAX_PERIOD:
            raise ValueError("step %s repeats only every %d frames (more than %d): round the rate or the speed" % (step, min(self.a, self.b), MAX_PERIOD))
        try:
            sigma = Fraction(1) if shutter is None else Fraction(shutter.strip() if isinstance(shutter, str) else shutter)
        except (ValueError, TypeError, ZeroDivisionError):
            raise ValueError("the shutter must be a number or a fraction (got %r)" % (shutter,)) from None
        if not 0 < sigma <= 1:
            raise ValueError("the shutter is the open fraction of the output frame's interval, in (0, 1] (got %s)" % sigma)
        if isinstance(samples, bool) or int(samples) != samples or samples < 1:
            raise ValueError("the shutter takes a whole number of samples, at least 1 (got %r)" % (samples,))
        self.shutter, self.samples = sigma, int(samples)
        self.p, self.qs = sigma.numerator, sigma.denominator * self.samples          # the grid: tau = m * gn / gd for m = k * qs + j * p
        g = step / self.qs
        self.gn, self.gd = g.numerator, g.denominator
        self.slots = self._slots()
        if max_slots is not None and self.slots > max_slots:
            if self.samples > 1:
                raise ValueError("step %s with a shutter of %s in %d samples puts %d sub-frames between two input frames; the plan takes at "
                                 "most %d (the largest upsample_rate - 1 at this pairs_per_batch)" % (step, sigma, self.samples, self.slots, max_slots))
            raise ValueError("step %s puts %d frames between two input frames; the plan takes at most %d (the largest upsample_rate - 1 at "
                             "this pairs_per_batch)" % (step, self.slots, max_slots))
        self._fed = self._k = 0

    def _slots(self):
        """The pattern of samples repeats every b outputs = a input frames (every output carries the same offsets j d).  Walk the shorter
        side: a pairs through the closed form, or the b * S samples of a period in time order - which without a shutter (S = 1) needs no
        walk: outputs more than a frame apart, a pair gets one at the most, and gets one unless every output is an input frame."""
        if self.a <= self.b:
            return max(self.count(i) for i in range(self.a))
        if self.samples == 1:
            return 1 if self.b > 1 else 0
        best = run = 0
        pair = -1
        for k in range(self.b):
            for i, t in self.samples_of(k):
                if not t:
                    continue
                run = run + 1 if i == pair else 1
                pair, best = i, max(best, run)
        return best

    def sample(self, k, j):
        """(i, t) of sub-frame j of output frame k."""
        i, r = divmod((k * self.qs + j * self.p) * self.gn, self.gd)
        return i, Fraction(r, self.gd)

    def samples_of(self, k):
        """The S (i, t) whose mean output frame k is, in time order."""
        return [self.sample(k, j) for j in range(self.samples)]

    def _upto(self, x, inclusive):
        """Samples at tau < x (or <= x) for an integer x: the grid points m <= mmax with m = k * qs + j * p, j < S."""
        mmax = (x * self.gd) // self.gn if inclusive else (x * self.gd - 1) // self.gn
        if mmax < 0:
            return 0
        k, r = divmod(mmax, self.qs)
        return k * self.samples + min(self.samples, r // self.p + 1)

    def on_frame(self, i):
        """(k, j) of the sample that is input frame i itself (t == 0), or None."""
        r = self._upto(i, False)
        return divmod(r, self.samples) if self._upto(i, True) > r else None

    def at(self, k):
        """(i, t) of output frame k: of its first sample."""
        return self.sample(k, 0)

    def n_outputs(self, n):
        """floor((n - 1) / step) + 1 output frames for n input frames; with a shutter, the k whose last sample is at n - 1 or before."""
        if n <= 0:
            return 0
        return max(0, (((n - 1) * self.gd) // self.gn - (self.samples - 1) * self.p) // self.qs + 1)

    def outputs(self, n):
        """[(i, t)] of every output frame of an n-frame clip; with a shutter, [the tuple of its S (i, t)]."""
        if self.samples > 1:
            return [tuple(self.samples_of(k)) for k in range(self.n_outputs(n))]
        return [self.at(k) for k in range(self.n_outputs(n))]

    def count(self, i):
        """Synthesised frames (with a shutter: samples) of pair (i, i + 1): those with i < tau < i + 1."""
        return self._upto(i + 1, False) - self._upto(i, True)

    def times(self, i):
        """The t of pair (i, i + 1)'s synthesised frames, increasing; with a shutter, (t, k, j) per synthesised sample."""
        r0 = self._upto(i, True)
        kjs = [divmod(r0 + m, self.samples) for m in range(self.count(i))]
        if self.samples > 1:
            return [(self.sample(*kj)[1],) + kj for kj in kjs]
        return [self.sample(*kj)[1] for kj in kjs]

    @staticmethod
    def t32(t):
        return np.float32(t.numerator / t.denominator)

    def feed(self, end=False):
        """The incremental form, for a pipe whose length nobody knows: call it once per frame read and once more, with end=True, at
        the end of the input.  Returns the [(i, t)] that have just become computable - an output needs frame i + 1 read, or frame i
        when t == 0, of its last sample - so the calls of an n-frame clip return outputs(n) piece by piece.  The call at the end returns nothing (what is
        left needs a frame that never came) and rewinds the timeline for the next clip."""
        if end:
            self._fed = self._k = 0
            return []
        self._fed += 1
        out = []
        while True:
            i, t = self.sample(self._k, self.samples - 1)          # the last sample decides: frame ceil(tau(k, S - 1)) has been read
            if i + (1 if t else 0) >= self._fed:
                return out
            out.append(tuple(self.samples_of(self._k)) if self.samples > 1 else (i, t))
            self._k += 1


class PassPlanner:
    """The bookkeeping of the timeline mode (_run_timeline), free of the GPU: which frames of the input stay in a ring slot's `cap` rows,
    which pairs a pass runs, and what the writer takes from the slot in the timeline's order.  read_passes reads each frame
    into row `rows` of the open slot and calls frame(); that returns None, or the closed slot as (order, pairs):
      order   [("interp", row of the slot's output buffer) | ("orig", row of its input buffer)], by increasing k
      pairs   [(row of the pair's first new payload, own_left, [fp32 times])] of at most pairs_per_batch pairs that run; pair p's frames
              are rows p * slots .. of the output buffer.  own_left: the pair's left frame is that row and its right frame the next
              one; otherwise the left frame is the right frame of the pair that ran before it (the one before in `pairs`, or the last
              of the pass before) and the row is the right frame's.
    end() closes what is open.  A frame that no output needs keeps no row: the next frame is read over it.  A frame that waits for its
    right neighbour stays in one slot with it: a slot closes at pairs_per_batch pairs, at cap rows, or one row early when no frame waits.
    closed_index: beside `pairs` of the slot closed last, the i of each of its pairs (i, i + 1) - what the scene cuts are reported by."""

    def __init__(self, tl, pairs_per_batch, cap):
        assert cap >= 2
        self.tl, self.pb, self.cap = tl, pairs_per_batch, cap
        self.f = 0                 # frames read
        self.prev_right = -1       # the input frame that the last running pair left on the device as its right frame
        self.closed_index = []
        self._open()

    def _open(self):
        self.rows, self.order, self.pairs, self._of, self._index = 0, [], [], None, []

    def _close(self):
        out = (self.order, self.pairs)
        self.closed_index = self._index
        self._open()
        return out

    def frame(self):
        tl, f, S = self.tl, self.f, self.tl.slots
        keep = tl.count(f) > 0          # the left frame of a pair that runs, if another frame follows
        for i, t in tl.feed():
            if t:                        # a frame of pair (f - 1, f)
                if self._of != i:
                    own_left = self.prev_right != i
                    assert not own_left or self.rows >= 1
                    self.pairs.append((self.rows - 1 if own_left else self.rows, own_left, []))
                    self._index.append(i)
                    self._of, self.prev_right = i, f
                self.order.append(("interp", (len(self.pairs) - 1) * S + len(self.pairs[-1][2])))
                self.pairs[-1][2].append(Timeline.t32(t))
            else:
                self.order.append(("orig", self.rows))
            keep = True
        self.rows += 1 if keep else 0
        waits = tl.count(f) > 0 and self.prev_right != f
        self.f += 1
        if len(self.pairs) == self.pb or self.rows == self.cap or (self.rows == self.cap - 1 and not waits):
            return self._close()
        return None

    def end(self):
        self.tl.feed(end=True)
        return self._close()


class GapTimeline:
    """The timeline of a clip whose repaired repeats are taken out (RepeatSource), over the frames that stay: frame i sits gap(i) input
    frames behind frame i - 1, and the output keeps the fixed grid of upsample_rate N on the INPUT's clock.  Pair (i - 1, i) with gap g
    gets g N - 1 synthesised frames at t = j / (g N), j = 1 .. g N - 1, and frame i follows as its own bytes: an ordinary pair (g = 1)
    gets the fixed grid's N - 1, a pair across a repaired run of m = g - 1 repeats fills the run's places as well.  It offers what
    PassPlanner asks of a Timeline - slots, count, times, feed - and nothing else of it; Timeline stays as it is.

    The gaps come in as they are decided: gap(g) once per frame that stays, in order, 0 for frame 0 (RepeatSource.on_gap), each before
    the frame to its left is fed - a planner asks count(i) when frame i has just been read, and a pair runs iff it gets a frame.  A gap
    not yet given counts as the end of the clip.  slots = (dedup_max + 1) N - 1, the most any pair can get; a plan that takes fewer is
    refused by D and N.  Memory: the gaps of the frames not yet fed, and one more."""

    def __init__(self, rate, dedup_max=DEDUP_MAX, max_slots=None):
        if isinstance(rate, bool) or int(rate) != rate or rate < 1:
            raise ValueError("with dedup the upsample_rate is a whole number of at least 1 (1: repair only; got %r)" % (rate,))
        self.rate, self.dedup_max = int(rate), parse_dedup_max(dedup_max)
        self.slots = (self.dedup_max + 1) * self.rate - 1
        if max_slots is not None and self.slots > max_slots:
            raise ValueError("dedup_max D = %d at upsample_rate N = %d puts up to (D + 1) N - 1 = %d frames between two input frames; the "
                             "plan takes at most %d (the largest upsample_rate - 1 at this pairs_per_batch): lower D or N"
                             % (self.dedup_max, self.rate, self.slots, max_slots))
        self._gaps, self._given, self._fed = {}, 0, 0

    def gap(self, g):
        """The gap in front of the next frame that stays: 0 for frame 0, then 1 .. dedup_max + 1."""
        assert (g == 0) == (self._given == 0) and 0 <= g <= self.dedup_max + 1, (g, self._given)
        self._gaps[self._given] = int(g)
        self._given += 1

    def count(self, i):
        """Synthesised frames of pair (i, i + 1): g N - 1 for its gap g; 0 where frame i + 1 is not known (the end of the clip)."""
        g = self._gaps.get(i + 1)
        return g * self.rate - 1 if g else 0

    def times(self, i):
        """The t of pair (i, i + 1)'s synthesised frames, increasing."""
        gn = self._gaps.get(i + 1, 0) * self.rate
        return [Fraction(j, gn) for j in range(1, gn)]

    t32 = staticmethod(Timeline.t32)

    def feed(self, end=False):
        """Timeline.feed over the frames that stay: once per frame read, the [(i, t)] that frame closes - the synthesised frames of the
        pair to its left, then the frame itself; end=True rewinds for the next clip."""
        if end:
            self._gaps, self._given, self._fed = {}, 0, 0
            return []
        f = self._fed
        out = [(f - 1, t) for t in self.times(f - 1)] if f else []
        self._gaps.pop(f - 1, None)
        self._fed += 1
        return out + [(f, Fraction(0))]


# One output is open at a time.  The samples in time order are the (k, j) in lexicographic order (Timeline), the accumulate calls follow
# that order within a pass and - through the event a pass waits for before its first one - from pass to pass, and an output is egressed
# right after its last call: the first call of output k + 1 (init = 1) comes after the egress of output k.  So between an output's first
# call and its egress no other output is touched, and the ring of accumulators needs this many entries.
OPEN_OUTPUTS = 1


class ShutterPlanner:
    """The bookkeeping of the shutter mode (_run_shutter), free of the GPU.  read_passes reads each frame into row `rows` of the
    open ring slot's input buffer and calls frame(); that returns None, or the closed pass as (rows, carry, pairs, calls, done):
      rows    the slot's first `rows` payloads go up and are ingested, in one piece, into rows 1 .. rows of the pass's planes
      carry   row 0 of the pass's planes is the last row of the pass before (that row's number, or None): the left frame of the first pair
      pairs   [(row of the left frame's planes, row of the right frame's, [fp32 times])] of at most pairs_per_batch pairs; pair p's
              synthesised frames are rows p * slots .. of the engine's output
      calls   the accumulate calls in time order: (src, first, count, k, init, last) with src = "frame" (row `first` of the planes, count
              1: a sample that is an input frame) or "interp" (`count` rows of the engine's output from row `first`: consecutive samples
              of one pair and one output); init on the first call of output k, last on its last: scale = fp32(1 / S), then egress
      done    the outputs that `calls` completes, increasing k: row o of the pass's output buffer is done[o]
    end() closes what is open.  Every frame that a sample needs - it is one, or it is the left or right frame of a pair that has one -
    takes a row, once; any other frame is read over by the next.  A pair runs in the pass that holds its right frame; its left frame
    is a row of that pass or `carry`.  A frame that is up only as a left frame stays in one pass with its right neighbour, so that it does
    not go up if that neighbour never comes: a pass closes at pairs_per_batch pairs, at cap rows, or one row early when no such frame
    waits.  Samples past the end of a clip whose output never completes are run and dropped: a pipe's length is not known ahead."""

    def __init__(self, tl, pairs_per_batch, cap):
        assert cap >= 2 and tl.samples > 1
        self.tl, self.pb, self.cap = tl, pairs_per_batch, cap
        self.max_done = (pairs_per_batch * tl.slots + cap + tl.samples - 1) // tl.samples      # of a run of that many samples, those with j = S - 1
        self.f = 0                 # frames read
        self.last = (-1, None)     # the newest frame that has planes on the device, and their row in the pass before
        self._rank = 0             # samples handed out: sample number r is (k, j) = divmod(r, S)
        self._open_k = None        # the output between its first call and its egress
        self._open()

    def _open(self):
        self.rows, self.carry, self.pairs, self.calls, self.done, self._row_of = 0, None, [], [], [], {}

    def _close(self):
        if self.rows:
            self.last = (self.last[0], self.rows)
        assert len(self.done) <= self.max_done and len(self.pairs) <= self.pb
        out = (self.rows, self.carry, self.pairs, self.calls, self.done)
        self._open()
        return out

    def _call(self, src, first, samples):
        """One accumulate call over `samples` = consecutive (k, j) of one output."""
        S = self.tl.samples
        k = samples[0][0]
        for kj in samples:
            assert kj == divmod(self._rank, S) and kj[0] == k, "samples are handed out in time order, none left out"
            self._rank += 1
        init, last = samples[0][1] == 0, samples[-1][1] == S - 1
        if init:
            assert self._open_k is None, "at most OPEN_OUTPUTS = 1 output is open"
            self._open_k = k
        assert self._open_k == k
        self.calls.append((src, first, len(samples), k, init, last))
        if last:
            self.done.append(k)
            self._open_k = None

    def frame(self):
        tl, f, slots = self.tl, self.f, self.tl.slots
        synth = tl.times(f - 1) if f else []
        here = tl.on_frame(f)
        if synth or here is not None or tl.count(f) > 0:
            self.rows += 1
            self._row_of[f] = self.rows
            if synth:                    # pair (f - 1, f): its left frame has planes, in this pass or as the last row of the one before
                if f - 1 not in self._row_of:
                    assert self.last[0] == f - 1 and self.last[1] is not None and self.carry is None
                    self.carry = self.last[1]
                    self._row_of[f - 1] = 0
                p = len(self.pairs)
                self.pairs.append((self._row_of[f - 1], self.rows, [Timeline.t32(t) for t, _, _ in synth]))
                m = 0
                while m < len(synth):          # one call per output the pair contributes to
                    e = m
                    while e < len(synth) and synth[e][1] == synth[m][1]:
                        e += 1
                    self._call("interp", p * slots + m, [kj[1:] for kj in synth[m:e]])
                    m = e
            if here is not None:
                self._call("frame", self.rows, [here])
            self.last = (f, None)
        waits = tl.count(f) > 0 and not synth and here is None          # up only as a left frame: it goes up with its right neighbour
        self.f += 1
        if len(self.pairs) == self.pb or self.rows == self.cap or (self.rows == self.cap - 1 and not waits):
            return self._close()
        return None

    def end(self):
        used = max([right for _, right, _ in self.pairs] + [first for src, first, _, _, _, _ in self.calls if src == "frame"], default=0)
        assert used >= self.rows - 1          # only the last row can be a left frame whose right neighbour never came: it stays down
        self.rows = used
        return self._close()


# ---- the streamed loop -------------------------------------------------------------------------------------------------------------
class _Drop:
    """The sink of a ring without a writer: the rows are taken and go nowhere."""

    def write_frame(self, buf):
        pass


_DROP = _Drop()


class PassRing:
    """The ring of `depth` slots between the loop that queues passes and the thread that writes what they made, and the loop's failure
    protocol.  Free of the GPU: an event is anything with synchronize(), the writer anything with write_frame(buf).

    The producer take()s a free slot, fills it and hand()s it over with the event that says its rows are there (None: nothing was queued
    on the GPU for it) and the row buffers to write, in order - or a callable that returns them, called on the thread once the event
    has come (the scene cuts: which rows are written depends on what the pass computed); a slot of None is an item that holds no slot
    (frame 0 of the fixed grid, written from a buffer of its own).  The thread (daemon, `y4m-writer`) waits for the event, writes the rows and frees the slot, item by
    item in the order handed over.  After the first exception on the thread nothing more is written and every slot handed over still
    comes back, so the producer never blocks in take(); it looks at `failure` and stops reading and submitting.  close() - leaving the
    `with` block - ends the thread, calls `settle` (the loop's device synchronise) and raises the stored exception, the object itself.
    An exception of the producer's own goes first: it propagates, and the ring shuts down under it without raising.
    writer None: the rows are taken, in order, and dropped (the hold-out scorer without an output, ssm_amd/video_score.py)."""

    def __init__(self, depth, writer, settle=None):
        self.writer, self.settle, self.failure = _DROP if writer is None else writer, settle, []
        self.free, self.work = queue.Queue(), queue.Queue()
        for r in range(depth):
            self.free.put(r)
        self.thread = threading.Thread(target=self._drain, name="y4m-writer", daemon=True)
        self.thread.start()

    def _drain(self):
        while True:
            item = self.work.get()
            if item is None:
                return
            r, event, rows = item
            try:
                if not self.failure:
                    if event is not None:
                        event.synchronize()
                    for buf in (rows() if callable(rows) else rows):
                        self.writer.write_frame(buf)
            except BaseException as e:          # noqa: BLE001 - handed to the caller's thread; keep releasing slots
                self.failure.append(e)
            if r is not None:
                self.free.put(r)

    def take(self, timeout=None):
        """A free slot; with a timeout (seconds), queue.Empty if none comes back in that time."""
        return self.free.get(timeout=timeout)

    def hand(self, r, event, rows):
        self.work.put((r, event, rows))

    def close(self, reraise=True):
        self.work.put(None)
        self.thread.join()
        if self.settle is not None:
            self.settle()
        if reraise and self.failure:
            raise self.failure[0]

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        self.close(reraise=exc_type is None)


def read_passes(reader, ring, plan, np_in, issue):
    """The read loop of the planner-driven modes (PassPlanner, ShutterPlanner): every frame of `reader` into row plan.rows of the open ring
    slot's input buffer; issue(slot, *closed) for every pass the planner closes, and for what is open at the end of the stream."""
    r = None
    while not ring.failure:
        if r is None:
            r = ring.take()
        if ring.failure or not reader.read_frame_into(np_in[r][plan.rows]):
            break
        closed = plan.frame()
        if closed is not None:
            issue(r, *closed)
            r = None
    if r is not None:
        issue(r, *plan.end())
    if plan.f == 0 and not ring.failure:
        raise Y4MError("the Y4M stream holds no frame")


def first_frame(reader, buf):
    """Frame 0 of a block mode into `buf`, ahead of its passes; a stream without one is refused."""
    if not reader.read_frame_into(buf):
        raise Y4MError("the Y4M stream holds no frame")


def read_blocks(ring, pb, np_in, read_unit, issue):
    """The read loop of the block modes (the fixed grid, the fields, video_score's hold-out scorer), whose passes are `pb` new units behind
    a carried one, frame 0 being the mode's own business: per pass a ring slot r and read_unit(r, i), i = 0 .. pb - 1, until it says that
    the stream has ended (for the interpolator one frame into np_in[r][i]; for the scorer a group of frames, the last of them there);
    then issue(r, valid) - also for the pass that found nothing, whose slot goes back empty.  A pass short of units is the last one, and
    its input rows are filled with copies of its last unit's: the engine runs on whole passes, what the extra pairs make is not written."""
    while not ring.failure:
        r = ring.take()
        valid = 0
        while valid < pb and read_unit(r, valid):
            valid += 1
        if 0 < valid < pb:
            np_in[r][valid:] = np_in[r][valid - 1]
        issue(r, valid)
        if valid < pb:
            return


def sad_runs(lefts, rights):
    """[(first pair, count)]: the pairs of a pass in maximal runs whose left rows and whose right rows both step evenly - what one
    ssm_luma_sad_fwd call addresses with its two strides.  One run whenever every pair of the pass follows the one before (the fixed
    grid, any slow motion) and for any two pairs; a timeline that skips pairs inside a pass of three or more may need a second call."""
    runs, p = [], 0
    while p < len(lefts):
        e = p + 1
        if e < len(lefts):
            da, db = lefts[e] - lefts[p], rights[e] - rights[p]
            e += 1
            while e < len(lefts) and (lefts[e] - lefts[e - 1], rights[e] - rights[e - 1]) == (da, db):
                e += 1
        runs.append((p, e - p))
        p = e
    return runs


def upload_times(times, slots, np_t, host_t, dev_t):
    """The engine's times of a pass, `slots` per pair: each pair's own (`times`: one list per pair), its last one repeated in the rest, and
    the last entry repeated after the last pair; filled into the ring slot's pinned buffer (host_t, np_t its numpy view) and queued for
    upload on the current stream - with the payloads, ahead of the kernels: see DESIGN 3.12."""
    for p, ts in enumerate(times):
        np_t[p * slots:p * slots + len(ts)] = ts
        np_t[p * slots + len(ts):(p + 1) * slots] = ts[-1]
    np_t[len(times) * slots:] = np_t[len(times) * slots - 1]
    dev_t.copy_(host_t, non_blocking=True)


RingSlots = namedtuple("RingSlots", "host_in host_out host_t np_in np_out np_t done")
StreamBuffers = namedtuple("StreamBuffers", "dev_in dev_out dev_t ingested dev_win")


def ring_slots(depth, fb, rows_in, rows_out, n_t=None, fb_out=None):
    """What a mode's `depth` ring slots hold, a RingSlots of lists: pinned host_in [rows_in, fb], host_out [rows_out, fb_out] (None: fb, one
    frame size for both) and host_t (n_t times, 0.5 throughout so that entries no pass fills stay finite; None where the mode has no
    times), their numpy views, the `done` events."""
    host_in, host_out = ([torch.empty(rows, size, dtype=torch.uint8).pin_memory() for _ in range(depth)]
                         for rows, size in ((rows_in, fb), (rows_out, fb if fb_out is None else fb_out)))
    host_t = None if n_t is None else [torch.full((n_t,), 0.5, dtype=torch.float32).pin_memory() for _ in range(depth)]
    np_in, np_out, np_t = (None if b is None else [t.numpy() for t in b] for b in (host_in, host_out, host_t))
    return RingSlots(host_in, host_out, host_t, np_in, np_out, np_t, [torch.cuda.Event() for _ in range(depth)])


def stream_buffers(n, dev, fb, rows_in, rows_out, n_t=None, fb_out=None):
    """What a mode's n streams hold on the device, a StreamBuffers of lists: dev_in, dev_out, dev_t (as in ring_slots; not initialised),
    `ingested`, and dev_win - None, or with fb_out, the window's size of a letterboxed clip, [rows_in, fb_out]: the scratch the cut windows
    of dev_in's rows go to, row for row; dev_out's rows are then of that size too."""
    dev_in, dev_out = ([torch.empty(rows, size, dtype=torch.uint8, device=dev) for _ in range(n)]
                       for rows, size in ((rows_in, fb), (rows_out, fb if fb_out is None else fb_out)))
    dev_t = None if n_t is None else [torch.empty(n_t, dtype=torch.float32, device=dev) for _ in range(n)]
    dev_win = None if fb_out is None else [torch.empty(rows_in, fb_out, dtype=torch.uint8, device=dev) for _ in range(n)]
    return StreamBuffers(dev_in, dev_out, dev_t, [torch.cuda.Event() for _ in range(n)], dev_win)


class PairOptions:
    """The per-pair options of one run of the fixed grid or of the timeline - scene cuts, static blocks, the window of a letterboxed clip,
    the flow check - in one place: what they add to the run's buffers, what they queue on a pass's stream, and what they decide on the
    writer thread.  With an option off nothing of it is allocated or queued, and with all of them off a pass is, launch for launch, the
    loop without them.
    flow_check = (T or None, alpha, beta): check_flow() scores the pass's pairs on the engine's own stage-1 planes behind the engine's run
    (ssm_flow_consistency_fwd), the eight words per pair go back to the ring slot like the block counts, and the writer thread notes
    every pair in the log's `flow_checks` and lets a pair with score >= T fall back like a cut pair (`flow_failed`).  It needs no row 0.
    flow_blocks = K (the flow check's per-block fallback): check_flow() also asks for the pairs' masks, one device mask [pairs, 2, h, w]
    per stream, and paste_flow() - behind the egress, ahead of paste_static() and of the copies to the host - lets ssm_flow_paste_fwd put
    the nearer frame's samples (flow_fallback "mix": ssm_flow_mix_fwd the cross-fade of the pair's two frames at the output's time) into
    every block with more than K inconsistent pixels; the failed blocks per pair go back to the ring
    slot like the static counts and the writer thread notes them in the log's `flow_repaired`.  It reads the pairs' payloads, so it
    needs row 0 as static blocks do.
    log: the VideoInterpolator whose `cuts` and `static` take the notes.

    Buffers (buffers()).  With scene cuts, static blocks or flow_blocks a stream's payload buffer has `lead` = 1 row in front of the pass's frames.  A pass
    names its pairs by rows of that buffer - pairs(k, lefts, rights): the fixed grid's are rows 0 .. pb - 1 against 1 .. pb, the timeline's
    whatever its planner kept - and row 0 stands for the right frame of the pair that ran last in the pass before, the left frame of this
    pass's first pair unless that pair brought its own.  The luma sums and the block counts of a pass sit per stream on the device and per
    ring slot in pinned memory; the counts go back behind the paste calls, the sums (download()) behind the pass's frames, both ahead of `done`.  With a window the frames
    come up into dev_up and Clip.ingest cuts their windows into dev_in, row for row, which is what everything here reads; without one
    dev_up is dev_in.

    Row 0 is carried by one of two protocols; why each is safe is said here and nowhere else.
      Scene cuts alone FORWARD it: ssm_luma_sad_fwd runs ahead of the pass's `ingested`, and behind its calls - still ahead of that
      record - pairs() copies the Y plane of the pass's last right frame into row 0 of the NEXT stream's buffer.  The pass that reads the
      row waits for that `ingested` before it ingests; the pass that read the row before, on that same next stream, recorded its own
      `ingested` - behind its calls - earlier in the chain of waits that this pass stands behind.  The fixed grid seeds it from frame 0.
      Static blocks and flow_blocks FETCH it (and with scene cuts too the fetched row serves the luma sums as well): ssm_static_paste_fwd
      and ssm_flow_paste_fwd read a pair's payloads behind the egress, long after the pass has recorded `ingested`, so no other stream
      may write the row.  Both pastes run on the pass's own stream and only read dev_in: the flow paste adds a reader of the row, at the
      same place in the stream's order as the static paste's, and no writer - so what makes the fetch safe for one makes it safe for both.  carry_in() copies
      the whole frame on the pass's own stream from row `last_right` of the stream before - behind a wait for that stream's `ingested`,
      ahead of the pass's own uploads; with one stream the source is the stream's own row, read before the uploads overwrite it.  The source
      row is next written by the upload of pass j + n - 1, which stands behind a chain of waits that ends at this pass's `ingested`,
      recorded after the fetch.

    The writer thread (rows() -> written()): PassRing calls it once the pass's event has come.  It notes the pass's block counts in
    `static`, feeds SceneCuts the luma sums in the order the pairs ran and notes the cuts, then yields the pass's rows: an input frame as
    it is; a synthesised frame of a cut pair replaced, whole, by the nearer input frame (t < 1/2: the left one); any other synthesised
    frame as it is or, with a window, pasted into the nearer input frame's bars (one buffer, written before the next is asked for).  At
    the end `carried`, the writer thread's copy of the frame that row 0 stands for, takes the last pair's right frame: its ring slot is
    free by the time the next pass's rows are written."""

    def __init__(self, log, clip, scene_cut=None, static=None, flow_check=None, flow_blocks=None, flow_fallback="nearer"):
        self.log, self.clip, self.static, self.flow, self.flow_blocks = log, clip, static, flow_check, flow_blocks
        assert flow_blocks is None or flow_check is not None, "flow_blocks is the flow check's"
        assert flow_fallback in FLOW_FALLBACKS and (flow_blocks is not None or flow_fallback == "nearer"), "flow_fallback is flow_blocks'"
        self.flow_mix = flow_fallback == "mix"          # a launch of another kernel on the same operands: nothing more is allocated
        self.fetch = static is not None or flow_blocks is not None          # a paste behind the egress reads the pair's payloads: row 0 is fetched
        self.cuts = None if scene_cut is None else SceneCuts(scene_cut)
        self.pixels, self.blocks = clip.h * clip.w, static_blocks(clip.h, clip.w)
        self.lead = 0 if self.cuts is None and not self.fetch else 1
        # the writer thread looks at a pair's input frames
        self.near = self.cuts is not None or clip.window is not None or (flow_check is not None and flow_check[0] is not None)
        self.carried = np.empty(clip.fb, np.uint8) if self.near else None
        self.paste, self.last_right = None, 0
        if clip.window is not None:
            out = np.empty(clip.fb_in, np.uint8)
            self.paste = lambda window, near: paste_window_host(window, near, *clip.frame, clip.siting, clip.bits, clip.window, out=out)

    def buffers(self, n, depth, pairs, rows_in, rows_out, n_t=None):
        """-> the StreamBuffers of n streams whose passes take rows_in payload rows (behind `lead`) and `pairs` pairs, on `depth` ring slots."""
        clip = self.clip
        sb = stream_buffers(n, clip.dev, clip.fb, self.lead + rows_in, rows_out, n_t, None if clip.window is None else clip.fb_out)
        self.n, self.ingested, self.dev_up, self.dev_in = n, sb.ingested, sb.dev_in, sb.dev_in if sb.dev_win is None else sb.dev_win

        def words():
            host = [torch.empty(pairs, dtype=torch.int64).pin_memory() for _ in range(depth)]
            return [torch.empty(pairs, dtype=torch.int64, device=clip.dev) for _ in range(n)], host, [t.numpy().view(np.uint64) for t in host]

        if self.cuts is not None:
            self.dev_sums, self.host_sums, self.np_sums = words()
        if self.static is not None:
            self.dev_counts, self.host_counts, self.np_counts = words()
        if self.flow is not None:
            self.dev_flow = [torch.empty(pairs, 2, 4, dtype=torch.float64, device=clip.dev) for _ in range(n)]
            self.host_flow = [torch.empty(pairs, 2, 4, dtype=torch.float64).pin_memory() for _ in range(depth)]
            self.np_flow = [t.numpy() for t in self.host_flow]
            nbytes = hb.load().ssm_flow_consistency_workspace_bytes(pairs, clip.h, clip.w)
            self.flow_ws = [torch.empty(nbytes, dtype=torch.uint8, device=clip.dev) for _ in range(n)]
        self.dev_mask = None
        if self.flow_blocks is not None:
            self.dev_mask = [torch.empty(pairs, 2, clip.h, clip.w, dtype=torch.uint8, device=clip.dev) for _ in range(n)]
            self.dev_failed, self.host_failed, self.np_failed = words()
        return sb

    def seed(self, frame, k, row, fetch_row):
        """Frame 0 of the fixed grid - `frame` on the host, row `row` of dev_in[k] on the current stream, ahead of `ingested` - as the
        frame that pass 0's row 0 stands for: where pass 0 fetches it (fetch_row: the last row, where every later pass leaves its own),
        or forwarded."""
        if self.carried is not None:
            self.carried[:] = frame
        if self.fetch:
            if fetch_row != row:
                self.dev_in[k][fetch_row].copy_(self.dev_in[k][row])
            self.last_right = fetch_row
        elif self.cuts is not None:
            self.dev_in[(k + 1) % self.n][0, :self.pixels].copy_(self.dev_in[k][row, :self.pixels])

    def carry_in(self, st, k, kprev, waited=False):
        """Ahead of the pass's uploads, the fetch of row 0; waited: the stream stands behind ingested[kprev] already."""
        if self.fetch:
            if not waited:
                st.wait_event(self.ingested[kprev])
            self.dev_in[k][0].copy_(self.dev_in[kprev][self.last_right])

    def pairs(self, k, lefts, rights):
        """Behind the pass's ingest and ahead of its `ingested`: the pass's pairs as rows of dev_in[k]; one ssm_luma_sad_fwd call per
        sad_runs run, and the forwarding of row 0."""
        self.lefts, self.rights, self.last_right = lefts, rights, rights[-1]
        if self.cuts is not None:
            d = self.dev_in[k]
            for p, m in sad_runs(lefts, rights):
                da, db = (lefts[p + 1] - lefts[p], rights[p + 1] - rights[p]) if m > 1 else (1, 1)
                luma_sad(d[lefts[p]:lefts[p] + (m - 1) * da + 1:da], d[rights[p]:rights[p] + (m - 1) * db + 1:db], self.clip.h, self.clip.w,
                         out=self.dev_sums[k][p:p + m])
            if not self.fetch:
                self.dev_in[(k + 1) % self.n][0, :self.pixels].copy_(d[rights[-1], :self.pixels])

    def paste_static(self, r, k, groups):
        """Behind the egress and ahead of the D2H copies of the frames: one ssm_static_paste_fwd call per group (first pair, pairs whose
        rows follow one another, their outputs [pairs * T, frame bytes]) that the mode names, then the counts' way back to ring slot r."""
        if self.static is not None:
            clip, d = self.clip, self.dev_in[k]
            for p, m, outputs in groups:
                static_paste(d[self.lefts[p]:self.lefts[p] + m], d[self.rights[p]:self.rights[p] + m], outputs, clip.h, clip.w, clip.siting,
                             clip.bits, self.static, counts=self.dev_counts[k][p:p + m])
            self.host_counts[r].copy_(self.dev_counts[k], non_blocking=True)

    def paste_flow(self, r, k, groups):
        """Behind the egress, ahead of paste_static and of the D2H copies of the frames: one ssm_flow_paste_fwd call per group (first
        pair, pairs whose rows follow one another, their outputs [pairs * T, frame bytes], the outputs of a pair that take the left
        frame) on the masks check_flow left, then the counts' way back to ring slot r.  With the fallback "mix" the call is
        ssm_flow_mix_fwd and a group's last entry the (num0, num_step, den) of a pair's times in place of the split.  With static too
        the static paste comes last: a static block's samples are the left frame's."""
        if self.flow_blocks is not None:
            clip, d = self.clip, self.dev_in[k]
            for p, m, outputs, at in groups:
                a, b, mask, counts = d[self.lefts[p]:self.lefts[p] + m], d[self.rights[p]:self.rights[p] + m], self.dev_mask[k][p:p + m], \
                    self.dev_failed[k][p:p + m]
                if self.flow_mix:
                    flow_mix(a, b, outputs, mask, clip.h, clip.w, clip.siting, clip.bits, self.flow_blocks, *at, counts=counts)
                else:
                    flow_paste(a, b, outputs, mask, clip.h, clip.w, clip.siting, clip.bits, self.flow_blocks, at, counts=counts)
            self.host_failed[r].copy_(self.dev_failed[k], non_blocking=True)

    def check_flow(self, r, k, flow4):
        """Behind the engine's run and ahead of the D2H copies of the frames: one ssm_flow_consistency_fwd call over the pass's pairs on
        flow4, the four planes F01 | F10 where the engine's stage 1 left them (PairEngine.s1.t["out"]), on the clip's picture inside the
        canvas; then the eight words per pair on their way back to ring slot r."""
        if self.flow is not None:
            from .flow_eval import flow_consistency
            clip, (_, alpha, beta) = self.clip, self.flow
            flow_consistency(flow4, clip.h, clip.w, *clip.at, alpha, beta, out=self.dev_flow[k], workspace=self.flow_ws[k],
                             want_mask=False if self.dev_mask is None else self.dev_mask[k])
            self.host_flow[r].copy_(self.dev_flow[k], non_blocking=True)

    def download(self, r, k):
        """Behind the D2H copies of the frames and ahead of `done`: the luma sums' way back to ring slot r."""
        if self.cuts is not None:
            self.host_sums[r].copy_(self.dev_sums[k], non_blocking=True)

    def rows(self, r, index, rows, near):
        """What PassRing.hand takes for a pass on ring slot r.  index: the clip's i of its pairs (i, i + 1) in the order they ran; rows: its
        buffers in write order; near() -> (pairs, at), asked for only where the writer thread looks at input frames: [(i, the left frame's
        host bytes or None for `carried`, the right frame's)] and per row None for an input frame or (pair's place in `pairs`, exact t).
        With every option off: `rows` itself."""
        if not self.near and self.static is None and self.flow is None:
            return rows
        pairs, at = near() if self.near else ((), [None] * len(rows))
        return functools.partial(self.written, list(index), self.np_sums[r] if self.cuts is not None else None,
                                 self.np_counts[r] if self.static is not None else None, pairs, list(zip(rows, at)),
                                 self.np_flow[r] if self.flow is not None else None,
                                 self.np_failed[r] if self.flow_blocks is not None else None)

    def written(self, index, sums, counts, pairs, order, flows=None, failed=None):
        """The generator behind rows(); sums, counts, flows: the pass's words in its ring slot, None with the option off.  A pair's
        synthesised frames fall back to the nearer input frame if it is a cut or fails the flow check."""
        if counts is not None:
            self.log.static.extend((i, int(counts[p]), self.blocks) for p, i in enumerate(index))
        if failed is not None:
            self.log.flow_repaired.extend((i, int(failed[p]), self.blocks) for p, i in enumerate(index))
        verdict = [False] * len(index)
        if sums is not None:
            for p, i in enumerate(index):
                verdict[p], score = self.cuts.feed(int(sums[p]), self.pixels)
                if verdict[p]:
                    self.log.cuts.append((i, score))
        if flows is not None:
            from .flow_eval import FlowCheck
            for p, i in enumerate(index):
                check = FlowCheck.of(flows[p])
                self.log.flow_checks.append((i, check))
                if self.flow[0] is not None and check.score >= self.flow[0]:
                    verdict[p] = True
                    self.log.flow_failed.append((i, check))
        for buf, at in order:
            if at is not None and (verdict[at[0]] or self.paste is not None):
                _, lf, rt = pairs[at[0]]
                near = (self.carried if lf is None else lf) if at[1] < Fraction(1, 2) else rt
                buf = near if verdict[at[0]] else self.paste(buf, near)
            yield buf
        if pairs:
            self.carried[:] = pairs[-1][2]


FieldProbe = namedtuple("FieldProbe", "verdict counts kinds order note warning advice")          # VideoInterpolator.field_probe


# Which options go together: one table for VideoInterpolator and for scripts/interpolate_video.py.
# OPTIONS, option: (as VideoInterpolator's messages spell it, as the command line's do, the value that says "not given" besides None).
# A spelling of None: that front end cannot be given the option; one with a % carries the value.
OPTIONS = {k: (k, "--" + k, None) for k in ("upsample_rate", "speed", "shutter", "scene_cut", "deinterlace", "dedup", "active", "field_probe",
                                            "static", "flow_check", "tile")}
OPTIONS.update({
    "target_rate": ("target_rate", "--fps", None), "slowmo": (None, "--slowmo", False), "recurrent": ("a recurrent model", None, False),
    "detelecine": ("detelecine", "--detelecine", False),          # no argument of the constructor: probe_fields meets it as a TelecineSource
    "shutter_light": ("shutter_light=%r", "--shutter_light %s", "coded"),
    "shutter_window": ("shutter_window=%r", "--shutter_window %s", None),          # both front ends hand a box over as None
    "flow_alpha": ("flow_alpha", None, None), "flow_beta": ("flow_beta", None, None), "flow_scale": ("flow_scale=%d", "--flow_scale %d", 1)})
_API, _FLAG = "{x} together with {y} is not available", "{x} does not go together with {y}"
_BETWEEN = "synthesised between two input frames"
_ACTIVE = ": the picture is cut out and the bars are pasted back around frames %s, and nothing else; chain two runs" % _BETWEEN
_STATIC = ": blocks that do not change are kept in frames %s as they were read, and nothing else; chain two runs" % _BETWEEN
_FLOW = ": it scores the two full-size stage-1 flows of a pair whose frames are %s, and nothing else" % _BETWEEN
_PROBE = ": a telecined clip is a mixture of progressive and combed frames by construction, and pulldown removal finds its field order itself"
_TIMELINE = " set the output's timeline themselves: they do not go together with --upsample_rate or --slowmo"
# OPTION_RULES, row: (options, others, needs, VideoInterpolator's message, the command line's).  With needs False the row refuses: it
# speaks when one of its options is given together with one of the others - {x} and {y} are the first given of each, as OPTIONS spells
# them.  With needs True it speaks when one of its options is given and none of the others.  A message of None: that front end has no
# such rule.  The first row that speaks supplies the message, so a pair may stand in one direction only (static names active, active
# does not name static) and a row may rest on the rows before it (shutter_timeline on shutter).  The rows are in the order in which
# VideoInterpolator asks them; FLAG_ORDER is the command line's.
OPTION_RULES = {
    "dedup": (("dedup",), ("target_rate", "speed", "shutter", "scene_cut", "deinterlace", "recurrent"), False,
              _API + ": it repairs repeated frames on the fixed grid of upsample_rate and nothing else; chain two runs (dedup with "
              "upsample_rate=1 first, then the other)",
              _FLAG + ": it repairs repeated frames on the grid of --upsample_rate and nothing else; pipe the output of --dedup "
              "--upsample_rate 1 into a second run"),
    "active": (("active",), ("shutter", "deinterlace", "dedup", "recurrent"), False, _API + _ACTIVE, _FLAG + _ACTIVE),
    "static": (("static",), ("shutter", "deinterlace", "dedup", "active", "recurrent"), False, _API + _STATIC, _FLAG + _STATIC),
    "flow_check": (("flow_check",), ("shutter", "deinterlace", "dedup", "flow_scale", "tile", "recurrent"), False, _API + _FLOW, _FLAG + _FLOW),
    "flow_numbers": (("flow_alpha", "flow_beta"), ("flow_check",), True,
                     "flow_alpha / flow_beta are the flow check's numbers: give flow_check, or leave them out", None),
    "field_probe": (("field_probe",), ("recurrent",), False, _API, None),
    "field_probe_detelecine": (("field_probe",), ("detelecine",), False, _API + _PROBE, _FLAG + _PROBE),
    "detelecine": (("detelecine",), ("deinterlace",), False, None,
                   _FLAG + ": pulldown removal pairs the fields of a film frame again, deinterlacing writes every field as a frame of its own"),
    "deinterlace": (("deinterlace",), ("upsample_rate", "slowmo", "target_rate", "speed", "shutter", "scene_cut", "recurrent"), False,
                    _API + ": deinterlacing writes the clip's fields as frames at twice its rate and nothing else; retime its progressive "
                    "output in a second run",
                    _FLAG + ": it writes the clip's fields as frames at twice its rate and nothing else; pipe its output into a second run "
                    "to retime it"),
    "shutter_light": (("shutter_light",), ("shutter",), True,
                      "{x} is the light in which a shutter averages: give a shutter, or leave it at \"coded\"",
                      "{x} is the light in which --shutter averages: it needs --shutter"),
    "shutter_window": (("shutter_window",), ("shutter",), True,
                       "{x} is the window of a shutter's sub-frames: give a shutter, or leave it at \"box\"",
                       "{x} is the window of the sub-frames that --shutter averages: it needs --shutter"),
    "scene_cut": (("scene_cut",), ("shutter",), False,
                  "{x} together with {y} is not defined: an average of sub-frames across a cut needs a definition of its own; give one of the two",
                  _FLAG + ": an average of sub-frames across a cut needs a definition of its own"),
    "shutter": (("shutter",), ("target_rate", "speed"), True,
                "a shutter averages over the interval of an output frame of target_rate / speed: give one of them (speed=1 keeps the "
                "input's rate)",
                "--shutter averages over the interval of an output frame of --fps / --speed: it needs one of them, and does not go together "
                "with --upsample_rate or --slowmo"),
    "shutter_timeline": (("shutter",), ("upsample_rate", "slowmo"), False, None, "--fps / --speed / --shutter" + _TIMELINE),   # behind "shutter"
    "timeline": (("target_rate", "speed"), ("upsample_rate", "slowmo"), False, None, "--fps / --speed" + _TIMELINE),
}
FLAG_ORDER = ("flow_check", "static", "field_probe_detelecine", "active", "dedup", "detelecine", "deinterlace", "shutter", "shutter_timeline",
              "timeline", "shutter_light", "shutter_window", "scene_cut")


def api_refusal(values, front=0, order=OPTION_RULES):
    """Why VideoInterpolator does not take the options `values` = {option of OPTIONS: value} together - the message of the first row
    that speaks - or None.  An option is given unless its value is None or the one OPTIONS names."""
    given = {k: OPTIONS[k][front] % (v,) if "%" in OPTIONS[k][front] else OPTIONS[k][front]          # option: as the message spells it
             for k, v in values.items() if k in OPTIONS and OPTIONS[k][front] is not None and v is not None and v != OPTIONS[k][2]}
    for row in order:
        options, others, needs, *texts = OPTION_RULES[row]
        x, y = (next((given[k] for k in names if k in given), None) for names in (options, others))
        if texts[front] is not None and x is not None and (y is None) == needs:
            return texts[front].format(x=x, y=y)
    return None


def flag_refusal(values):
    """The same for the command line's flags, in its own order of asking."""
    return api_refusal(values, 1, FLAG_ORDER)


class VideoInterpolator:
    """reader -> (upsample_rate - 1) frames between every two input frames -> writer, streamed; or, with target_rate / speed, the frames
    of a Timeline (any output rate, any speed: _run_timeline).

    A pass takes `pairs_per_batch` new frames: H2D of their payloads, ingest (each frame once: its planes are the right frame of one
    pair and, carried over, the left frame of the next), the PairPipeline engine of the pass's stream, egress, D2H into the pass's slot
    of a ring of pinned buffers - all queued on that stream, nothing synchronises the host inside the loop but the ring itself.  A
    writer thread waits for a slot's event and writes, per pair, the interpolated frames and then the right frame's own input bytes.
    Host and device memory are fixed by the frame size, n_streams and pairs_per_batch.

    The four modes (_run_fixed, _run_timeline, _run_shutter, _run_fields) share what is not on a stream: the prologue (_clip) and the Clip's two
    conversions, the allocation of what a ring slot and a stream hold (ring_slots, stream_buffers), the ring with its writer thread and
    failure protocol (PassRing), the read loops (read_passes for the planners, read_blocks for the fixed grid and the fields) and the
    issue of passes (_run_passes), the fill of a pass's times (upload_times); the fixed grid and the timeline drive one PairOptions for
    scene cuts, static blocks and the letterbox window.  Each keeps its own submit: what is queued on a pass's stream, call for call, is what its bytes and its rate rest on."""

    def __init__(self, model, cfg, upsample_rate=None, n_streams=2, pairs_per_batch=1, matrix=None, color_range=None, flow_scale=1,
                 tile=None, halo=256, blend=32, target_rate=None, speed=None, shutter=None, shutter_samples=8, scene_cut=None,
                 shutter_light="coded", deinterlace=None, dedup=None, dedup_max=DEDUP_MAX, active=None, active_probe=ACTIVE_PROBE,
                 shutter_window="box", field_probe=None, static=None, flow_check=None, flow_alpha=None, flow_beta=None,
                 flow_blocks=None, flow_fallback="nearer"):
        """target_rate = (num, den) and / or speed (a Fraction, or what Fraction() takes; 1/4 is four times slower): the output follows
        Timeline(speed * input rate / target_rate) instead of the fixed grid of upsample_rate, which is then not used (see
        _run_timeline); with both None nothing changes.  flow_scale = 2 or 4: the coarse-flow mode of FullModel.interpolate (U-Nets at 1/flow_scale of the size; an approximation of the
        reference's output, not parity); the canvas is then padded to multiples of 32 * flow_scale.  tile = (th, tw): the tiled mode of
        FullModel.interpolate (windows of tile + halo stitched with a cross-fade of `blend`; an approximation of the untiled output,
        not parity).
        shutter (a Fraction in (0, 1], or what Fraction() takes: the open fraction of the output frame's interval, 1/2 = 180 degrees),
        beside target_rate or speed: every output frame is the mean of shutter_samples sub-frames over that part of its interval
        (Timeline, _run_shutter).  Like the command line's --shutter it needs one of the two, since it averages over the interval of
        their timeline; speed=1 is the input's own rate with blur.  The 8 samples of the default are a convention, not backed by a
        measurement of quality.  shutter_samples = 1, or shutter None, is the loop without a shutter.
        shutter_light ("coded", or the name of one of LIGHT_CURVES: "bt709", "srgb", "bt1886"), with a shutter: "coded" is the mean of
        the gamma-coded R'G'B' values, launch for launch the loop as it was before the option.  A curve makes it the mean of light, what
        a sensor integrates: every sub-frame is denormalised, clamped to [0, 1] - a synthesised value outside counts as 0 or 1, where the
        coded mean lets it cancel - and decoded before it is added, and the mean is encoded again (ssm_frames_accumulate_light_fwd).
        Which curve is right depends on how the clip was graded (bt709 for camera-referred material, srgb or bt1886 for material
        mastered on a display), which no Y4M header says: so the choice is the user's and the default stays "coded".  It acts on
        R'G'B' after the matrix and is independent of matrix and color_range.  "pq" and "hlg" (HDR_LIGHTS) are the BT.2100 transfer
        functions of HDR clips, the same way through ssm_frames_accumulate_hdr_fwd: pq the PQ EOTF (display light as a fraction of
        10000 cd/m2), hlg the inverse of the HLG OETF (scene light), neither with an OOTF.
        shutter_window ("box", "triangle", "hann", "gauss" or "gauss:K"; parse_shutter_window), with a shutter: the weights of an
        output's sub-frames.  "box" weighs them alike and is, launch for launch, the loop as it was before the option.  The others fall
        off towards the ends of the exposure (shutter_window(name, shutter_samples)): the S evenly bright copies of a fast object become
        a streak that fades in and out, at the same S and so the same stage-2 cost; every accumulate call is then the weighted sibling
        of the one above (ssm_frames_accumulate_weighted_fwd and its light and HDR forms) with its slice of the window, and the output
        closes with the window's scale in place of 1 / S.  It goes with every shutter_light.  gauss spans +-K standard deviations;
        K = 2, like the 8 samples, is a convention.  With shutter_samples = 1 any window is the loop without a shutter.
        matrix (None: default_matrix(h) per clip; BT601, BT709 or BT2020 = MATRICES' values): BT2020 is never a default, since no Y4M
        header names the matrix.
        scene_cut (a Fraction in (0, 1], or what Fraction() takes; no default value): the threshold of SceneCuts.  Every pass then also
        sums the luma differences of its pairs on the GPU, and at a pair that SceneCuts calls a cut the writer puts out, instead of the
        synthesised frames, the left input frame's own bytes at t < 1/2 and the right one's from there on; `cuts` lists (i, score) of
        every cut pair (i, i + 1) after run().  The pair still runs on the GPU.  Not together with a shutter: an average across a cut
        needs a definition of its own.  None: the loop as it is without the option, launch for launch.
        upsample_rate None is 8.
        deinterlace ("auto", "tff", "bff"; _run_fields): the clip is interlaced, and its n frames come out as 2n progressive frames at twice
        the rate (field_outputs).  "auto" takes the field order from the reader's header (a Y4MReader(interlaced=True)) and refuses Ip and
        I?; "tff" and "bff" override any header.  The fields run through the fixed grid of upsample_rate = 2 at t = 1/2, at half the
        frame's height: matrix (None: default_matrix of the FRAME's height), color_range, flow_scale and tile / halo / blend act as
        they do there.  To retime the progressive output, chain a second run.  None: every other mode as it is.
        dedup (True: the default thresholds at the clip's depth; or (hi, lo, frac) / "HI:LO:FRAC", parse_dedup) with dedup_max = D:
        frames that repeat the one before (Repeats, from the 8 x 8 block differences of ssm_block_sad_fwd) in runs of at most D are
        repaired - the output keeps the fixed grid of upsample_rate, and the places of a run's repeats and of the frames around them
        are filled by frames synthesised between the run's two neighbours (GapTimeline; a RepeatSource in front of the timeline
        mode's loop).  upsample_rate = 1 is then legal and means repair only.  `repeats` lists the runs after run(): (first repeat, m,
        repaired, worst max, worst over).  The defaults are the numbers of ffmpeg's mpdecimate, a convention, not its construction and
        not backed by a measurement on compressed footage.  None: every mode as it is, launch for launch.
        active ("auto", "auto:LIM[:FRAC]", "W:H:X:Y" or (w, h, x, y); parse_active) with active_probe = P: the clip is letterboxed, and
        the run is that of its picture alone.  The rectangle is the one given, or with "auto" the smallest aligned one that holds every
        active row and column of the first P frames (ActiveArea, from the counts of ssm_luma_counts_fwd; an ActiveSource in front of the
        loop).  Every pass cuts the rectangle out of its uploaded frames on the device (ssm_window_cut_fwd) and runs canvas, plan and
        launches of the cropped clip; only window bytes come back, and the writer thread pastes each synthesised window into the bytes
        of the nearer input frame (t < 1/2: the left one), so the bars - and a subtitle in them - step with their own frames, the rule of
        the scene cuts.  Input frames stay their own bytes, whole.  The default matrix is that of the FRAME's height.  After run():
        `active` is the rectangle used, (w, h, x, y), or None where the run went whole-frame (the rectangle is the frame, no probed frame
        has an active line, or it is under 32 samples in a direction - then byte for byte the run without the option), `active_note` one
        line that says which and why, `active_excess` [(frame index, active rows outside, active columns outside)] of later frames that
        leave the rectangle; they are reported and change nothing.  LIM = 24 at 8 bits is the number of ffmpeg cropdetect's limit, not
        its construction, FRAC = 1/64 this module's own: conventions, not backed by a measurement on compressed footage.  With a
        shutter every output comes from the accumulator, and none has one input frame's bars.  None: every mode as it is, launch for
        launch.
        field_probe (True: FIELD_PROBE = 48 frames; or P, parse_field_probe): the field order is looked for in the data.  A
        FieldOrderSource in front of the loop takes the comb sums of the first P frames on the GPU (ssm_field_order_sums_fwd) and decides
        "tff", "bff", "progressive" or nothing (FieldVerdict).  With deinterlace="auto" and a header that says Ip or I? the run takes the
        verdict as its field order, and refuses by name, before anything is written, a verdict of "progressive" or none - the message
        carries the four counts and says to give "tff" or "bff".  With a header that says It or Ib, and with "tff" / "bff", the order is
        what it is without the option, and a verdict that contradicts it is a warning that changes nothing.  Without deinterlace it is a
        report, and the clip runs as it does without the option.  After run() (or probe_fields()): `field_probe`, a FieldProbe of
        verdict, counts (nT, nB, nP, nU), kinds, order (the order in use, None without deinterlace), note (one line with the counts),
        warning (the contradiction, or None) and advice (a report-only run on a clip that looks interlaced: the line that names
        deinterlace="tff" / "bff"; else None).  The ratios are conventions in the spirit of ffmpeg's idet, not its construction, and not
        backed by a measurement on noisy or compressed footage.  Frames behind the probe are not watched.  probe_fields refuses a
        TelecineSource: a telecined clip is a mixture of both kinds of frame by construction.  None: every mode as it is, launch for
        launch.
        static (LO, a whole number in 0 .. 2^24 - 1, or its text; parse_static; no default value): blocks that do not change keep their
        bytes.  Where the two frames of a pair agree on an 8 x 8 block - the sum of |difference| over its luma and the chroma under it is
        at most LO, in codes of the clip's depth - every frame synthesised between them carries the LEFT frame's samples of that block
        (static_paste_host is the definition; ssm_static_paste_fwd does it on the pass's stream, behind the egress and ahead of the copy
        to the host, on the payloads as they were uploaded).  0 is exact: both neighbours hold those samples, so no honest in-between
        frame differs there - a logo, subtitles, a timecode, a locked-off background stop pulsing against the input frames' own bytes.
        Any other LO is the user's number.  Not claimed: a block that agrees in both frames while something crossed it in between is
        kept; the seams between kept and synthesised blocks are not smoothed.  After run(): `static` lists (i, static blocks, blocks) of
        every pair (i, i + 1) that got outputs.  With scene_cut a cut pair's outputs are replaced whole, as without static; with a shutter
        every output is an accumulator's.  Every format is taken.  None: every mode as it is, launch for launch.
        flow_check (True: a report; or a threshold T >= 0, a Fraction or what flow_eval.parse_flow_check takes, "T" or "T:ALPHA:BETA"; no
        default T) with flow_alpha, flow_beta (None: flow_eval.FLOW_ALPHA, FLOW_BETA = 0.01 and 0.5, the numbers of Sundaram, Brox and
        Keutzer 2010 - a convention, not backed by a measurement here): every pass then also scores the forward-backward consistency of
        its pairs' two stage-1 flows on the GPU (ssm_flow_consistency_fwd on the engine's own planes, on the clip's picture, behind the
        engine's run and ahead of the copies to the host), eight words per pair.  After run(): `flow_checks` lists (i, FlowCheck) of every
        pair (i, i + 1) that ran.  With a threshold a pair whose FlowCheck.score - the larger share of inconsistent among the judged
        pixels of the two directions, a Fraction - is >= T falls back like a cut pair: the left input frame's bytes at t < 1/2, the right
        one's from there on; `flow_failed` lists those pairs.  Scores lie in [0, 1]: T = 0 condemns every pair, any T > 1 none.  The
        pair still runs on the GPU.  With this repository's synthetic weights a score says nothing about quality.  With scene_cut a pair
        falls back if it is a cut or fails the check.  Every format is taken.  None: every mode as it is, launch for launch - nothing
        is allocated or queued.
        flow_blocks (K, a whole number in 0 .. 64; parse_flow_blocks; no default value), a sub-option of flow_check like dedup_max of
        dedup: the per-block fallback.  Every pass then also takes the pairs' masks from the check and, behind the egress and ahead of
        the copy to the host (and ahead of the static paste), ssm_flow_paste_fwd puts the NEARER input frame's samples - the left
        frame's at t < 1/2, the right one's from there on - into every 8 x 8 block (static's blocks) of a synthesised frame in which
        more than K of the 64 luma pixels are inconsistent in at least one direction (flow_paste_host is the definition).  K = 64 fails
        nothing and is the run without it, byte for byte; K = 0 fails every block with one inconsistent pixel.  After run():
        `flow_repaired` lists (i, failed blocks, blocks) of every pair (i, i + 1) that got outputs.  flow_check=True with flow_blocks is
        the report plus the per-block fallback, no pair-level T; with a T a pair that reaches it - or, with scene_cut, a cut pair - is
        still replaced whole.  Not claimed: K has no default; seams between pasted and synthesised blocks are not smoothed; a block from
        the nearer frame inside a moving region steps rather than moves; with this repository's synthetic weights nothing can be said
        about quality.  Not together with active (chain two runs).  None: the run with flow_check as it is, launch for launch.
        flow_fallback ("nearer" or "mix"; parse_flow_fallback), a sub-option of flow_blocks: what a failed block carries.  "nearer" is
        the run as described above, launch for launch.  "mix": ssm_flow_mix_fwd in place of ssm_flow_paste_fwd, on the same masks, at
        the same place in the pass - every sample of a failed block is a (1 - t) + b t of the pair's two frames at the output's EXACT
        time t, rounded half up (flow_mix_host is the definition): (j + 1) / upsample_rate on the fixed grid, on a timeline the
        output's own Fraction over the denominator of the timeline's step, which is at most 65535 (flow_mix_den; a larger one is
        refused by name before anything is written; 24 -> 59.94 gives 2500, 29.97 -> 25 gives 1001).  A pair that reaches flow_check's
        T, and a cut pair, are still replaced whole by the NEARER frame; with static the static paste still comes last;
        `flow_repaired` keeps its meaning.  Not claimed: where "nearer" steps, "mix" ghosts; which looks better is not known, and
        cannot be with synthetic weights; there is still no default K; seams are not smoothed.  Without flow_blocks "mix" is refused.
        Which of these options do not go together, which need another, and what each refusal says is one table, OPTION_RULES (above
        the class; api_refusal asks it here, flag_refusal for the command line), not a list kept per option."""
        from .coarse import check_scale
        from .flow_eval import FLOW_ALPHA, FLOW_BETA, parse_flow_check
        from .tiles import check_args
        self.flow_scale = check_scale(flow_scale)
        if self.flow_scale != 1 and getattr(model, "recurrent", False):
            raise NotImplementedError("flow_scale=%d is not available with a recurrent bottleneck" % self.flow_scale)
        self.tile, self.halo, self.blend = (None, halo, blend) if tile is None else check_args(tile, halo, blend)
        if self.tile is not None and self.flow_scale != 1:
            raise NotImplementedError("tile=%dx%d together with flow_scale=%d: tiles are not available in the coarse-flow mode"
                                      % (self.tile + (self.flow_scale,)))
        if self.tile is not None and getattr(model, "recurrent", False):
            raise NotImplementedError("tile=%dx%d is not available with a recurrent bottleneck" % self.tile)
        n_frames = cfg.getint("TRAIN", "N_FRAMES")
        if n_frames != 2:
            raise NotImplementedError("N_FRAMES=%d needs the recurrent bottleneck (unpinned upstream); use N_FRAMES=2" % n_frames)
        self.dedup = None if dedup is None or dedup is False else parse_dedup(dedup)
        self.dedup_max = parse_dedup_max(dedup_max)
        self.active_option, self.active_probe = parse_active(active), parse_active_probe(active_probe)
        self.static_lo = None if static is None else parse_static(static)
        self.flow_check = None
        if flow_check is not None and flow_check is not False:
            t, a, b = parse_flow_check(flow_check, flow_alpha, flow_beta)
            self.flow_check = (t, float(FLOW_ALPHA if a is None else a), float(FLOW_BETA if b is None else b))
        self.field_probe_option = None if field_probe is None or field_probe is False else (
            FIELD_PROBE if field_probe is True else parse_field_probe(field_probe))
        self.field_probe, self._probed, self._probed_order = None, None, None
        self.deinterlace = parse_deinterlace(deinterlace)
        rate = 8 if upsample_rate is None else upsample_rate
        if int(rate) < (2 if self.dedup is None else 1):
            raise ValueError("upsample_rate must be at least 2" if self.dedup is None else "upsample_rate must be at least 1 with dedup")
        self.model, self.cfg, self.rate = model, cfg, int(rate)
        self.n_streams, self.pb = max(1, int(n_streams)), max(1, int(pairs_per_batch))
        if matrix is not None:
            table_index(matrix)          # refuses an unknown matrix by name, here rather than at the first clip
        self.matrix, self.color_range = matrix, color_range
        self._pipe = None
        self.target_rate = None if target_rate is None else parse_rate("%s:%s" % tuple(target_rate))
        self.speed = None if speed is None else parse_speed(speed)
        self.shutter, self.samples = (None, 1) if shutter is None else (shutter, shutter_samples)
        if shutter is not None:
            Timeline(1, shutter=shutter, samples=shutter_samples)          # refuses a bad value by name, here rather than at the first clip
        self.shutter_light = parse_shutter_light(shutter_light)
        self.shutter_window = parse_shutter_window(shutter_window)
        self.timed = target_rate is not None or speed is not None
        self.scene_cut = None if scene_cut is None else parse_scene_cut(scene_cut)
        refusal = api_refusal(dict(
            upsample_rate=upsample_rate, target_rate=target_rate, speed=speed, shutter=shutter, scene_cut=self.scene_cut,
            shutter_light=shutter_light, shutter_window=None if self.shutter_window[0] == "box" else shutter_window,
            deinterlace=self.deinterlace, dedup=self.dedup, active=self.active_option, field_probe=self.field_probe_option,
            static=self.static_lo, flow_check=self.flow_check, flow_alpha=flow_alpha, flow_beta=flow_beta, flow_scale=self.flow_scale,
            tile=self.tile, recurrent=getattr(model, "recurrent", False)))
        if refusal is not None:          # every value has been through its own check: what is left is which options go together
            raise ValueError(refusal)
        self.flow_blocks = None          # a sub-option of the flow check, not a row of the table: its own refusals, after the table's
        if flow_blocks is not None:
            if self.flow_check is None:
                raise ValueError("flow_blocks is the flow check's per-block fallback: give flow_check, or leave it out")
            if self.active_option is not None:
                raise ValueError("flow_blocks together with active is not available: the blocks of the per-block fallback are the whole "
                                 "frame's, not a cut window's; chain two runs")
            self.flow_blocks = parse_flow_blocks(flow_blocks)
        self.flow_fallback = parse_flow_fallback(flow_fallback)          # flow_blocks' own sub-option: what a failed block carries
        if self.flow_fallback != "nearer" and self.flow_blocks is None:
            raise ValueError("flow_fallback=\"%s\" is what a failed block of flow_blocks carries: give flow_blocks, or leave it out"
                             % self.flow_fallback)
        self._new_log()

    def _new_log(self):
        """What a run reports (the constructor's docstring names each), empty: the state before a run and at the start of every run()."""
        self.cuts, self.repeats, self.static, self.flow_checks, self.flow_failed, self.flow_repaired = [], [], [], [], [], []
        self.active, self.active_note, self.active_excess = None, None, []

    def canvas(self, h, w):
        """(Hp, Wp) of the planes an h x w clip runs on: padded_dims to multiples of 32 * flow_scale."""
        return padded_dims(h, w, 32 * self.flow_scale)[0]

    def timeline(self, in_rate):
        """The Timeline of a clip at `in_rate` (num, den); refuses a step whose slots the plan would not take and, with
        flow_fallback="mix", one whose denominator ssm_flow_mix_fwd does not take (flow_mix_den)."""
        tl = Timeline(timeline_step(in_rate, self.target_rate, self.speed), max_slots=MAX_STAGE2_BATCH // self.pb, shutter=self.shutter,
                      samples=self.samples)
        if self.flow_fallback == "mix":
            flow_mix_den(tl)
        return tl

    def gap_timeline(self):
        """The GapTimeline of a run with dedup; refuses a dedup_max and upsample_rate whose slots the plan would not take."""
        return GapTimeline(self.rate, self.dedup_max, max_slots=MAX_STAGE2_BATCH // self.pb)

    def _pipeline(self, hp, wp, dev, n_t=None):          # n_t None: the fixed grid's upsample_rate - 1
        import os
        from .engine import PairPipeline
        m = self.model
        mode = m.precision or os.environ.get("SSM_PRECISION", sys.modules[type(m).__module__].DEFAULT_PRECISION)      # as FullModel.interpolate
        n_t = self.rate - 1 if n_t is None else n_t
        key = (hp, wp, str(dev), mode, self.n_streams, self.pb, n_t, self.flow_scale, self.tile, self.halo, self.blend, m._stamp())
        if self._pipe is None or self._pipe[0] != key:
            sd1 = {k: v.detach() for k, v in m.stage1_model.state_dict().items()}
            sd2 = {k: v.detach() for k, v in m.stage2_model.state_dict().items()}
            self._pipe = None
            self._pipe = (key, PairPipeline(sd1, sd2, n_t, hp, wp, dev, m.cross_skip, mode, self.n_streams,
                                            pairs_per_batch=self.pb, flow_scale=self.flow_scale, tile=self.tile, halo=self.halo,
                                            blend=self.blend))
        return self._pipe[1]

    def _model_device(self):
        dev = next(self.model.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("the model must be on the GPU (the HIP path has no CPU fallback)")
        return dev

    def _clip(self, reader, writer, window=None):
        """The Clip of a run, or the refusal of a writer of another format or of a model that is not on the GPU.  window: the active area of
        a letterboxed clip; the default matrix stays the one of the frame's height."""
        h, w, siting, bits = reader.height, reader.width, reader.siting, getattr(reader, "bits", 8)
        if (writer.height, writer.width, writer.siting, getattr(writer, "bits", 8)) != (h, w, siting, bits):
            raise ValueError("reader and writer disagree on the frame format")
        if self.scene_cut is not None and bits > 8:
            raise ValueError("scene_cut is not available for C%s: the luma differences (ssm_luma_sad_fwd) and the score's / 255 are for 8-bit "
                             "samples, these have %d bits" % (reader.chroma, bits))
        matrix = default_matrix(h) if self.matrix is None else self.matrix
        crange = self.color_range if self.color_range is not None else (reader.color_range if reader.color_range is not None else LIMITED)
        return Clip(h, w, siting, matrix, crange, self.cfg, bits, 32 * self.flow_scale, dev=self._model_device(), window=window)

    def probe_fields(self, reader):
        """The reader behind a FieldOrderSource that has decided (the option field_probe), for run(): sets `field_probe` and the field
        order of a deinterlace="auto" run on a header without one, or refuses it.  run() calls it on a reader that has not been through
        it; a caller that opens its writer only after the refusals calls it first."""
        assert self.field_probe_option is not None, "probe_fields is the option field_probe's"
        if isinstance(reader, TelecineSource):
            raise ValueError(api_refusal({"field_probe": self.field_probe_option, "detelecine": True}))
        source = FieldOrderSource(reader, self._model_device(), self.field_probe_option)
        verdict = source.decide()
        order = warning = advice = None
        self._probed_order = None
        if self.deinterlace is not None:
            if self.deinterlace == "auto" and source.interlace not in FIELD_ORDERS:
                if verdict not in ("tff", "bff"):
                    raise ValueError("deinterlace=\"auto\" on a header that says I%s takes the field order from the field probe, and the probe "
                                     "says %s (%s): give deinterlace=\"tff\" or \"bff\""
                                     % (source.interlace, "the clip is progressive" if verdict == "progressive" else "nothing", source.note))
                order = self._probed_order = verdict
            else:
                order = field_order(self.deinterlace, source.interlace)
                if verdict is not None and verdict != order:
                    warning = "field probe: the data says %s, the run is %s as %s says; nothing changes" % (
                        verdict, order, "the header (I%s)" % source.interlace if self.deinterlace == "auto" else "the option")
        elif verdict in ("tff", "bff"):
            advice = "field probe: the clip looks interlaced, %s: --deinterlace %s (deinterlace=\"%s\") writes its fields as frames" % (
                "top field first" if verdict == "tff" else "bottom field first", verdict, verdict)
        self.field_probe = FieldProbe(verdict, source.counts, source.kinds, order, source.note, warning, advice)
        self._probed = source
        return source

    @torch.no_grad()
    def run(self, reader, writer):
        """Returns the number of frames written: (n - 1) * upsample_rate + 1 for n input frames (with target_rate / speed:
        floor((n - 1) / step) + 1; with a shutter: Timeline.n_outputs(n); with deinterlace: 2 n; with dedup the fixed grid's count)."""
        self._new_log()
        if self.flow_fallback == "mix" and self.timed:
            self.timeline(reader.rate)          # a denominator that ssm_flow_mix_fwd does not take: refused before a frame is read or written
        if self.field_probe_option is not None and reader is not self._probed:
            reader = self.probe_fields(reader)
        self._probed = None          # one run per probe
        if self.active_option is not None:
            reader = ActiveSource(reader, self._model_device(), self.active_option, self.active_probe)
            self.active, self.active_note, self.active_excess = reader.decide(), reader.note, reader.excess
        clip = self._clip(reader, writer, self.active)
        if self.dedup is not None:
            tl = self.gap_timeline()
            source = RepeatSource(reader, clip.dev, self.dedup, self.dedup_max)
            source.on_gap, self.repeats = tl.gap, source.repeats
            return self._run_timeline(clip, source, writer, tl)
        if self.deinterlace is not None:
            return self._run_fields(clip, reader, writer)
        if not self.timed:
            return self._run_fixed(clip, reader, writer)
        return self._run_shutter(clip, reader, writer) if self.samples > 1 else self._run_timeline(clip, reader, writer)

    def _run_passes(self, clip, writer, done, read, has_work, submit, rows_of, first=None, last=None):
        """The loop of every mode, over the passes that read(ring, issue) closes - read_passes with a mode's planner, read_blocks with its
        unit reader: has_work(*closed) - the pass has GPU work; submit(j, r, *closed) queues it as pass j on ring slot r; rows_of(r, on_gpu,
        *closed) -> (the rows to write as PassRing.hand takes them, their number).  first(ring), last(ring): what a mode hands to the ring
        ahead of pass 0 and, unless the writer has failed, behind the last pass; each returns the number of its frames."""
        written = j = 0          # frames written, passes issued

        def issue(r, *closed):
            nonlocal written, j
            on_gpu = has_work(*closed) and not ring.failure
            if on_gpu:
                submit(j, r, *closed)
                j += 1
            rows, count = rows_of(r, on_gpu, *closed)
            ring.hand(r, done[r] if on_gpu else None, rows)
            written += count

        with PassRing(len(done), writer, lambda: torch.cuda.synchronize(clip.dev)) as ring:
            if first is not None:
                written += first(ring)
            read(ring, issue)
            if last is not None and not ring.failure:
                written += last(ring)
        return written

    def _run_fixed(self, clip, reader, writer):
        """run() on the fixed grid of upsample_rate: planes[k] is [carried left frame | pairs_per_batch new frames], the pairs an
        overlapping view of it; the times go up once per run.  Frame 0 is written from a pinned buffer of its own before any pass, and
        ingested where pass 0 looks for its carried left frame.  The passes are read_blocks': a short last one runs whole, its extra
        pairs are not written.

        The per-pair options are PairOptions': with scene_cut or static a stream's payload buffer has one row in front, the left payloads
        of a pass's pairs are rows 0 .. pb - 1 and the right ones rows 1 .. pb, so one ssm_luma_sad_fwd call and one ssm_static_paste_fwd
        call (T = upsample_rate - 1 outputs a pair) take them all; a pass fetches its row 0 from row pb of the stream before."""
        from .evaluation import t_values
        fb, dev, hp, wp = clip.fb, clip.dev, clip.hp, clip.wp
        pipe = self._pipeline(hp, wp, dev)
        n, pb, nt = pipe.n, self.pb, self.rate - 1
        depth = n + 2                                                  # ring slots: one per pass in flight, one being read, one being written
        t_dev = torch.tensor(t_values(self.rate), dtype=torch.float32, device=dev)
        slots = ring_slots(depth, fb, pb, pb * nt, fb_out=clip.fb_out)
        np_in, np_out = slots.np_in, slots.np_out
        opt = PairOptions(self, clip, self.scene_cut, self.static_lo, self.flow_check, self.flow_blocks, self.flow_fallback)
        lead, lefts, rights = opt.lead, list(range(pb)), list(range(1, pb + 1))
        flow_at = fixed_mix(self.rate) if opt.flow_mix else fixed_split(self.rate)          # what a failed block takes in a pair's outputs
        _, dev_out, _, ingested, _ = opt.buffers(n, depth, pb, pb, pb * nt)
        planes = [torch.empty(pb + 1, 3, hp, wp, dtype=torch.float32, device=dev) for _ in range(n)]      # [carried left frame | new frames]
        first = torch.empty(1, fb, dtype=torch.uint8).pin_memory()
        first_frame(reader, first.numpy()[0])
        torch.cuda.synchronize(dev)
        pairs_done = 0

        def frame0(ring):
            ring.hand(None, None, [first.numpy()[0]])
            last = (n - 1) % n
            with torch.cuda.stream(pipe.streams[last]):
                up, new = opt.dev_up[last][lead:lead + 1], opt.dev_in[last][lead:lead + 1]
                up.copy_(first, non_blocking=True)
                clip.ingest(up, planes[last][pb:], scratch=new)
                opt.seed(first.numpy()[0], last, lead, pb)
                ingested[last].record()
            return 1

        def submit(j, r, valid):
            k, kprev = j % n, (j - 1) % n
            st = pipe.streams[k]
            with torch.cuda.stream(st):
                opt.carry_in(st, k, kprev)
                opt.dev_up[k][lead:].copy_(slots.host_in[r], non_blocking=True)
                st.wait_event(ingested[kprev])
                planes[k][0].copy_(planes[kprev][pb])
                clip.ingest(opt.dev_up[k][lead:], planes[k][1:], scratch=opt.dev_in[k][lead:])
                opt.pairs(k, lefts, rights)
                ingested[k].record()
                x = planes[k]
                img6 = x.view(1, 6, hp, wp) if pb == 1 else x.as_strided((pb, 6, hp, wp), (3 * hp * wp, hp * wp, wp, 1))
                frames = pipe.engines[k].run(img6, t_dev, False)
                opt.check_flow(r, k, pipe.engines[k].s1.t["out"] if opt.flow is not None else None)
                clip.egress(frames, dev_out[k])
                opt.paste_flow(r, k, [(0, pb, dev_out[k], flow_at)])
                opt.paste_static(r, k, [(0, pb, dev_out[k])])
                slots.host_out[r].copy_(dev_out[k], non_blocking=True)
                opt.download(r, k)
                slots.done[r].record()

        def rows_of(r, on_gpu, valid):
            nonlocal pairs_done
            i0, pairs_done = pairs_done, pairs_done + valid
            order = list(pass_order(valid, nt))
            rows = [np_out[r][row] if kind == "interp" else np_in[r][row] for kind, row in order]

            def near():
                return ([(i0 + p, np_in[r][p - 1] if p else None, np_in[r][p]) for p in range(valid)],
                        [None if kind == "orig" else (row // nt, Fraction(row % nt + 1, self.rate)) for kind, row in order])

            return (opt.rows(r, range(i0, i0 + valid), rows, near) if on_gpu else rows), valid * self.rate

        return self._run_passes(clip, writer, slots.done, lambda ring, issue: read_blocks(
            ring, pb, np_in, lambda r, i: reader.read_frame_into(np_in[r][i]), issue), lambda valid: valid > 0, submit, rows_of, first=frame0)

    def _run_fields(self, clip, reader, writer):
        """run() with deinterlace: the n interlaced frames come out as the 2n progressive frames of field_outputs - the fixed grid of
        upsample_rate = 2 run on the clip's two parity streams, between two byte-moving kernels.

        A pass takes pairs_per_batch new frames and makes two outputs per frame.  On its stream: H2D of the frames (once); the field
        payloads of the pass, rows [2 carried | top, bottom of every new frame], by one ssm_fields_split_fwd; every new field ingested
        once at half the frame's height into fplanes[k][parity] = [carried left field | the new ones] - it is the right operand of one
        pair now, the left one of the next pass's after the copy on the device, and its payload is the kept half of one output; per parity
        one engine run at t = 1/2 over the pass's pairs of that parity, exactly the fixed grid's call, and the egress of its frames into
        the rows of `made` of the outputs they belong to; then ssm_fields_weave_fwd from the field payloads (kept) and `made` into whole
        frames, and D2H.  Output 2m - 1 keeps the later field of frame m - 1 and takes the other rows from the pair of the EARLIER
        fields of frames m - 1 and m; output 2m keeps the earlier field of frame m and takes the pair of the later fields.  Under tff
        the kept fields of a pass are consecutive rows and one weave call takes them; under bff they are, per frame, rows 3 apart: one
        call of N = 2 per frame.  Output 0 (with frame 0, ahead of the passes) and output 2n - 1 (after the last) are woven with
        fill = 1 from their own field alone.  Every output frame comes from the GPU; memory is fixed by the frame size, n_streams and
        pairs_per_batch."""
        from .evaluation import t_values
        h, w, bits = clip.h, clip.w, getattr(reader, "bits", 8)
        crange, siting = clip.coding[2:4]
        order = (self._probed_order if self.field_probe_option is not None else None) or field_order(self.deinterlace, reader.interlace)
        fh, _ = field_dims(h, w, siting)
        matrix = default_matrix(h) if self.matrix is None else self.matrix          # of the frame's height, not the field's
        fclip = Clip(fh, w, siting, matrix, crange, self.cfg, bits, 32 * self.flow_scale, dev=clip.dev)
        fb, hfb, dev, hp, wp = clip.fb, fclip.fb, clip.dev, fclip.hp, fclip.wp
        pipe = self._pipeline(hp, wp, dev, 1)
        n, pb = pipe.n, self.pb
        depth = n + 2
        early, late = field_of(0, order)[1], field_of(1, order)[1]          # the parities of a frame's earlier and later field
        t_dev = torch.tensor(t_values(2), dtype=torch.float32, device=dev)
        host_in, host_out, _, np_in, np_out, _, done = ring_slots(depth, fb, pb, 2 * pb)
        dev_in, dev_out, _, ingested, _ = stream_buffers(n, dev, fb, pb, 2 * pb)
        fields = [torch.empty(2 + 2 * pb, hfb, dtype=torch.uint8, device=dev) for _ in range(n)]      # row 2 (1 + i) + parity: frame i of the pass; i = -1 carried
        made = [torch.empty(2 * pb, hfb, dtype=torch.uint8, device=dev) for _ in range(n)]
        fplanes = [torch.empty(2, pb + 1, 3, hp, wp, dtype=torch.float32, device=dev) for _ in range(n)]      # [parity][carried left field | new ones]
        # the kept fields of a pass's outputs as (first row of `fields`, rows between one and the next, count, first output): see above
        runs = [(1, 1, 2 * pb, 0)] if order == "tff" else [(2 * i, 3, 2, 2 * i) for i in range(pb)]

        def weave(kept, mk, out, parity0, fill):
            fields_weave(kept, mk, h, w, siting, bits, parity0, fill, out=out)

        def split_ingest(k, frames, i0):
            """The frames' fields into rows 2 (1 + i0) .. of fields[k], and their planes behind the carried ones."""
            rows = fields[k][2 * (1 + i0):2 * (1 + i0 + frames.shape[0])]
            fields_split(frames, h, w, siting, bits, out=rows)
            for i in range(frames.shape[0]):
                for q in (TOP, BOTTOM):
                    fclip.ingest(rows[2 * i + q:2 * i + q + 1], fplanes[k][q, 1 + i0 + i:2 + i0 + i])

        first_in, first_out = (torch.empty(1, fb, dtype=torch.uint8).pin_memory() for _ in range(2))
        first_frame(reader, first_in.numpy()[0])
        torch.cuda.synchronize(dev)
        tail = ((n - 1) % n, pb - 1)          # stream and place of the newest frame: its later field closes the clip

        def frame0(ring):
            """Frame 0: split and ingested where pass 0 looks for its carried fields; output 0 from its earlier field alone."""
            last = tail[0]
            first_done = torch.cuda.Event()
            with torch.cuda.stream(pipe.streams[last]):
                dev_in[last][pb - 1:].copy_(first_in, non_blocking=True)
                split_ingest(last, dev_in[last][pb - 1:], pb - 1)
                weave(fields[last][2 * pb + early:2 * pb + early + 1], None, dev_out[last][:1], early, 1)
                first_out.copy_(dev_out[last][:1], non_blocking=True)
                ingested[last].record()
                first_done.record()
            ring.hand(None, first_done, [first_out.numpy()[0]])
            return 1

        def submit(j, r, valid):
            nonlocal tail
            k, kprev = j % n, (j - 1) % n
            st = pipe.streams[k]
            with torch.cuda.stream(st):
                dev_in[k].copy_(host_in[r], non_blocking=True)
                st.wait_event(ingested[kprev])          # the carried fields; and pass j - n + 1 is done with fields[k] and fplanes[k]
                fields[k][late].copy_(fields[kprev][2 * pb + late])
                fplanes[k][:, 0].copy_(fplanes[kprev][:, pb])
                split_ingest(k, dev_in[k], 0)
                ingested[k].record()
                for s, q in enumerate((early, late)):          # the pairs of the earlier fields make outputs 0, 2, .. of the pass
                    x = fplanes[k][q]
                    img6 = x.view(1, 6, hp, wp) if pb == 1 else x.as_strided((pb, 6, hp, wp), (3 * hp * wp, hp * wp, wp, 1))
                    frames = pipe.engines[k].run(img6, t_dev, False)
                    for i in range(pb):
                        fclip.egress(frames[i:i + 1], made[k][2 * i + s:2 * i + s + 1])
                for row, step, count, o in runs:
                    weave(fields[k][row:row + (count - 1) * step + 1:step], made[k][o:o + count], dev_out[k][o:o + count],
                          field_of(2 * j * pb + 1 + o, order)[1], 0)
                host_out[r].copy_(dev_out[k], non_blocking=True)
                done[r].record()
            tail = (k, valid - 1)

        def closing(ring):
            """Output 2n - 1: the later field of the last frame, alone."""
            r = ring.take()
            k, i = tail
            with torch.cuda.stream(pipe.streams[k]):
                weave(fields[k][2 * (1 + i) + late:2 * (1 + i) + late + 1], None, dev_out[k][:1], late, 1)
                host_out[r][:1].copy_(dev_out[k][:1], non_blocking=True)
                done[r].record()
            ring.hand(r, done[r], [np_out[r][0]])
            return 1

        return self._run_passes(clip, writer, done, lambda ring, issue: read_blocks(
            ring, pb, np_in, lambda r, i: reader.read_frame_into(np_in[r][i]), issue), lambda valid: valid > 0, submit,
            lambda r, on_gpu, valid: ([np_out[r][o] for o in range(2 * valid)], 2 * valid), first=frame0, last=closing)

    def _run_timeline(self, clip, reader, writer, tl=None):
        """run() with target_rate / speed: the output frames are those of Timeline(speed * reader.rate / target_rate); with dedup those of
        the GapTimeline `tl` over the frames that the RepeatSource `reader` hands on.

        Pairs now differ: pair (i, i + 1) gets tl.count(i) synthesised frames at its own times, and a pair that gets none is not run -
        no upload, no ingest, no stage 1 or 2, no egress.  A pass collects up to pairs_per_batch pairs that do run.  Every engine is
        planned for `slots` times per pair; a pair with m < slots runs with its last time repeated in the rest, only its first m
        frames go through the egress kernel and back to the host.  The times go up from a pinned buffer of the pass's ring slot on the
        pass's stream.  A ring slot holds `cap` input payloads - every frame read lands in one, a frame nobody needs is overwritten by
        the next - and the writer thread takes from it, in the timeline's order, rows of host_out ("interp") and of host_in ("orig").
        Each uploaded frame is ingested once: a pair's left frame is the previous running pair's right frame copied on the device, or,
        after a pair that did not run, ingested with the right one.  A pass short of pairs (end of clip, or a slot full of frames passed
        through) leaves the planes of its unused entries as they are: finite, and never read back.  Memory is fixed by the frame size,
        n_streams, pairs_per_batch and slots.

        The per-pair options are PairOptions', as on the fixed grid: row 0 in front of a stream's payloads stands for the right frame of the
        pair that ran last in the pass before; a pair's left payload is its own uploaded row, the right row of the pair before it, or row
        0.  The rows of the pairs that run step evenly unless the timeline skips pairs inside a pass (sad_runs): one ssm_luma_sad_fwd call
        then, one per run otherwise; only pairs that run are summed and fed to SceneCuts.  With static one ssm_static_paste_fwd call per
        pair, with T the number of its outputs, behind the pass's egress calls and ahead of its D2H copies."""
        fb, dev, hp, wp = clip.fb, clip.dev, clip.hp, clip.wp
        tl = self.timeline(reader.rate) if tl is None else tl
        S, pb, n = tl.slots, self.pb, self.n_streams
        pipe = self._pipeline(hp, wp, dev, S) if S else None          # an integer step only picks input frames: nothing to run
        depth, cap = n + 2, 2 * pb + 2
        host_in, host_out, host_t, np_in, np_out, np_t, done = ring_slots(depth, fb, cap, pb * max(S, 1), pb * max(S, 1), fb_out=clip.fb_out)
        plan = PassPlanner(tl, pb, cap)
        if pipe is not None:
            opt = PairOptions(self, clip, self.scene_cut, self.static_lo, self.flow_check, self.flow_blocks, self.flow_fallback)
            lead = opt.lead
            _, dev_out, dev_t, ingested, _ = opt.buffers(n, depth, pb, cap, pb * S, pb * S)
            planes = [torch.zeros(pb, 2, 3, hp, wp, dtype=torch.float32, device=dev) for _ in range(n)]      # [pair][left | right]
        torch.cuda.synchronize(dev)
        last_p = [0]          # place, in its pass, of the pair whose right frame the next pair may carry over

        def submit(j, r, order, pairs):
            """Pass j: `pairs` = [(first row of the pair's new payloads, the left frame is among them, its times)] of ring slot r."""
            k, kprev = j % n, (j - 1) % n
            st = pipe.streams[k]
            with torch.cuda.stream(st):
                if j:
                    st.wait_event(ingested[kprev])          # the carried frame; and pass j - n + 1 is done with planes[k]
                    opt.carry_in(st, k, kprev, waited=True)
                new, up = opt.dev_in[k][lead:], opt.dev_up[k][lead:]
                for p, (row, own_left, ts) in enumerate(pairs):
                    rows = 2 if own_left else 1
                    up[row:row + rows].copy_(host_in[r][row:row + rows], non_blocking=True)
                    if not own_left:
                        planes[k][p, 0].copy_(planes[k][p - 1, 1] if p else planes[kprev][last_p[0], 1])
                    clip.ingest(up[row:row + rows], planes[k][p, 2 - rows:], scratch=new[row:row + rows])
                upload_times([ts for _, _, ts in pairs], S, np_t[r], host_t[r], dev_t[k])
                rights = [lead + row + (1 if own_left else 0) for row, own_left, _ in pairs]          # rows of dev_in[k]
                lefts = [lead + row if own_left else (rights[p - 1] if p else 0) for p, (row, own_left, _) in enumerate(pairs)]
                opt.pairs(k, lefts, rights)
                ingested[k].record()
                last_p[0] = len(pairs) - 1
                frames = pipe.engines[k].run(planes[k].view(pb, 6, hp, wp), dev_t[k], False)
                opt.check_flow(r, k, pipe.engines[k].s1.t["out"] if opt.flow is not None else None)
                if all(len(ts) == S for _, _, ts in pairs):
                    spans = [(0, len(pairs) * S)]
                else:
                    spans = [(p * S, len(ts)) for p, (_, _, ts) in enumerate(pairs)]
                late = opt.fetch          # the pasted blocks stand between the egress calls and the copies of what they made
                for o, m in spans:
                    clip.egress(frames[o:o + m], dev_out[k][o:o + m])
                    if not late:
                        host_out[r][o:o + m].copy_(dev_out[k][o:o + m], non_blocking=True)
                if late:
                    if opt.flow_blocks is not None:          # exact times, as the writer thread's rule asks: t < 1/2 takes the left frame
                        exact = [tl.times(i) for i in plan.closed_index]
                        at = (lambda ts: times_mix(ts, tl.step.denominator)) if opt.flow_mix else times_split
                        opt.paste_flow(r, k, [(p, 1, dev_out[k][p * S:p * S + len(ts)], at(exact[p][:len(ts)]))
                                              for p, (_, _, ts) in enumerate(pairs)])
                    opt.paste_static(r, k, [(p, 1, dev_out[k][p * S:p * S + len(ts)]) for p, (_, _, ts) in enumerate(pairs)])
                    for o, m in spans:
                        host_out[r][o:o + m].copy_(dev_out[k][o:o + m], non_blocking=True)
                opt.download(r, k)
                done[r].record()

        def rows_of(r, on_gpu, order, pairs):
            rows = [np_out[r][row] if kind == "interp" else np_in[r][row] for kind, row in order]
            if not on_gpu:
                return rows, len(order)
            index = list(plan.closed_index)

            def near():
                exact = [tl.times(i) for i in index]          # the pairs' times as Fractions, beside the planner's fp32
                rights = [np_in[r][row + (1 if own_left else 0)] for row, own_left, _ in pairs]
                return ([(i, np_in[r][row] if own_left else (rights[p - 1] if p else None), rights[p])
                         for p, (i, (row, own_left, _)) in enumerate(zip(index, pairs))],
                        [None if kind == "orig" else (row // S, exact[row // S][row % S]) for kind, row in order])

            return opt.rows(r, index, rows, near), len(order)

        return self._run_passes(clip, writer, done, lambda ring, issue: read_passes(reader, ring, plan, np_in, issue),
                                lambda order, pairs: bool(pairs), submit, rows_of)

    def _run_shutter(self, clip, reader, writer):
        """run() with a shutter: output frame k is the mean of the S = shutter_samples sub-frames of Timeline(step, shutter=, samples=),
        summed in time order into an fp32 accumulator by ssm_frames_accumulate_fwd and egressed from it - every output, also one whose
        samples are all input frames.  With shutter_light a curve every one of those calls is ssm_frames_accumulate_light_fwd instead
        (ssm_frames_accumulate_hdr_fwd for "pq" and "hlg"),
        with encode = 1 on an output's last: the accumulator holds light in between and normalised coded planes for the egress.
        With a shutter_window other than "box" every call is the weighted sibling instead and carries w[j0 : j0 + count] of
        shutter_window(name, S), j0 the samples of the open output that earlier calls took (0 on init), and the last call the window's
        scale; a call of more than ACC_WEIGHTS_MAX samples goes out as consecutive pieces of at most that many - init on the first, scale
        and encode on the last - which is the same sum in the same order.  "box" makes none of these: today's calls, launch for launch.

        A pass (bookkeeping: ShutterPlanner) uploads and ingests, in one piece each, the frames it holds that a sample needs; copies the
        planes of up to pairs_per_batch pairs that get a sample side by side; runs them at their sample times padded to `slots`; and
        then makes its accumulate calls in time order - one per pair and output the pair contributes to, over that pair's consecutive
        frames of that output, and one of N = 1 on the ingested planes of a frame that is a sample itself - with init = 1 on an output's
        first call and scale = fp32(1 / S) on its last, after which the output is egressed from the accumulator and copied back in the
        same pass.  An output may span pairs, passes and streams: just before its first accumulate call a pass waits for the event that
        the pass before recorded after its last accumulate and egress, so the engines of neighbouring passes still overlap, only these
        short tails are serialised, and the result depends on nothing but the time order.  One output is open at a time (OPEN_OUTPUTS),
        which sizes the ring of accumulators.  Memory is fixed by the frame size, n_streams, pairs_per_batch, slots and that bound."""
        fb, dev, hp, wp = clip.fb, clip.dev, clip.hp, clip.wp
        tl = self.timeline(reader.rate)
        slots, pb, n = tl.slots, self.pb, self.n_streams
        pipe = self._pipeline(hp, wp, dev, slots) if slots else None          # a step whose samples are all input frames: nothing to synthesise
        streams = pipe.streams if pipe is not None else [torch.cuda.Stream(dev) for _ in range(n)]
        depth, cap = n + 2, 2 * pb + 2
        plan = ShutterPlanner(tl, pb, cap)
        scale = np.float32(1.0 / tl.samples)
        window = None          # "box": no weighted call
        if self.shutter_window[0] != "box":
            window, scale = shutter_window(self.shutter_window, tl.samples)
        light = hdr = None
        if self.shutter_light in HDR_KINDS:
            kind, row = hdr_light(self.shutter_light)
            hdr = (*clip.norm, kind, (ctypes.c_float * HDR_ROW)(*[float(x) for x in row]))
        elif self.shutter_light != "coded":
            light = (*clip.norm, (ctypes.c_float * LIGHT_ROW)(*[float(x) for x in light_curve(self.shutter_light)]))
        host_in, host_out, host_t, np_in, np_out, np_t, done = ring_slots(depth, fb, cap, plan.max_done, pb * max(slots, 1))
        dev_in, dev_out, dev_t, ingested, _ = stream_buffers(n, dev, fb, cap, plan.max_done, pb * max(slots, 1))
        planes = [torch.zeros(cap + 1, 3, hp, wp, dtype=torch.float32, device=dev) for _ in range(n)]      # [carried frame | the pass's frames]
        sides = [torch.zeros(pb, 2, 3, hp, wp, dtype=torch.float32, device=dev) for _ in range(n)]         # [pair][left | right]
        acc = torch.zeros(OPEN_OUTPUTS, 3, hp, wp, dtype=torch.float32, device=dev)
        summed = [torch.cuda.Event() for _ in range(n)]
        torch.cuda.synchronize(dev)

        taken = [0]          # samples of the open output that the calls so far took: where the next call's weights start in the window

        def accumulate_pieces(x, a, init, last, w):
            """One planner call with a window: the weighted entry point of the light, in pieces of at most ACC_WEIGHTS_MAX frames."""
            assert len(w) == x.shape[0], "a call's samples (%d) leave the window (%d weights left)" % (x.shape[0], len(w))
            for p0 in range(0, x.shape[0], ACC_WEIGHTS_MAX):
                p1 = min(p0 + ACC_WEIGHTS_MAX, x.shape[0])
                i, e, sc = 1 if init and p0 == 0 else 0, 1 if last and p1 == x.shape[0] else 0, scale if last and p1 == x.shape[0] else 1.0
                if hdr is not None:
                    hb.frames_accumulate_hdr(x[p0:p1], a, i, sc, *hdr, e, weights=w[p0:p1])
                elif light is None:
                    hb.frames_accumulate(x[p0:p1], a, i, sc, weights=w[p0:p1])
                else:
                    hb.frames_accumulate_light(x[p0:p1], a, i, sc, *light, e, weights=w[p0:p1])

        def submit(j, r, rows, carry, pairs, calls, finished):
            """Pass j on ring slot r; the arguments are ShutterPlanner's."""
            k, kprev = j % n, (j - 1) % n
            st = streams[k]
            with torch.cuda.stream(st):
                if j:
                    st.wait_event(ingested[kprev])          # the carried frame; and pass j - n + 1 is done with planes[k]
                dev_in[k][:rows].copy_(host_in[r][:rows], non_blocking=True)
                if carry is not None:
                    planes[k][0].copy_(planes[kprev][carry])
                clip.ingest(dev_in[k][:rows], planes[k][1:1 + rows])
                for p, (left, right, _) in enumerate(pairs):
                    sides[k][p, 0].copy_(planes[k][left])
                    sides[k][p, 1].copy_(planes[k][right])
                if pairs:
                    upload_times([ts for _, _, ts in pairs], slots, np_t[r], host_t[r], dev_t[k])
                ingested[k].record()
                frames = pipe.engines[k].run(sides[k].view(pb, 6, hp, wp), dev_t[k], False) if pairs else None
                if j:
                    st.wait_event(summed[kprev])          # the accumulator: every call and egress of the passes before, in time order
                o = 0
                for src, first, count, ko, init, last in calls:
                    a = acc[ko % OPEN_OUTPUTS:ko % OPEN_OUTPUTS + 1]
                    x = planes[k][first:first + 1] if src == "frame" else frames[first:first + count]
                    if window is not None:
                        taken[0] = 0 if init else taken[0]
                        accumulate_pieces(x, a, init, last, window[taken[0]:taken[0] + x.shape[0]])
                        taken[0] += x.shape[0]
                    elif hdr is not None:
                        hb.frames_accumulate_hdr(x, a, 1 if init else 0, scale if last else 1.0, *hdr, 1 if last else 0)
                    elif light is None:
                        hb.frames_accumulate(x, a, 1 if init else 0, scale if last else 1.0)
                    else:
                        hb.frames_accumulate_light(x, a, 1 if init else 0, scale if last else 1.0, *light, 1 if last else 0)
                    if last:
                        clip.egress(a, dev_out[k][o:o + 1])
                        host_out[r][o:o + 1].copy_(dev_out[k][o:o + 1], non_blocking=True)
                        o += 1
                summed[k].record()
                done[r].record()

        # a pass without GPU work: with no rows the planner has recorded no call, so `finished` is empty; after a failure the thread writes nothing
        return self._run_passes(clip, writer, done, lambda ring, issue: read_passes(reader, ring, plan, np_in, issue),
                                lambda rows, *_: rows > 0, submit,
                                lambda r, on_gpu, *closed: ([np_out[r][o] for o in range(len(closed[-1]))], len(closed[-1])))
