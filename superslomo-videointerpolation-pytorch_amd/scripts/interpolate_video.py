#!/usr/bin/env python3
"""Slow-motion video, streamed: a YUV4MPEG2 (.y4m) file or pipe in, one out, with upsample_rate - 1 interpolated frames between every two
input frames.  Y4M is the container every player and ffmpeg read and write without a codec, pipes included:

    ffmpeg -i clip.mp4 -f yuv4mpegpipe - | interpolate_video.py -c cfg.ini --expt e --log run.log --input - --output - | ffplay -

  Y4M payload -> pinned host memory -> GPU -> ingest kernel (chroma upsampling, range, matrix, normalise, pad to x32)   [ssm_amd.video]
      -> the pair pipeline (stage 1 once per pair, all t batched, passes on 2 HIP streams)
      -> egress kernel (crop, denormalise, matrix, chroma subsampling, range, rounding) -> pinned host memory -> Y4M payload

Memory does not grow with the clip (scripts/visualize_interpolation.py, the PNG tool, holds the whole clip on the GPU).  Input frames
pass to the output as their own bytes.  The output's frame rate is the input's times upsample_rate - the same duration, smoother - or,
with --slowmo, the input's: the same frames played upsample_rate times slower.  4:2:0 (both sitings), 4:2:2 and 4:4:4 at 8 bits per sample,
and C420pB, C422pB, C444pB at B = 9, 10, 12, 14 or 16 (what `ffmpeg -f yuv4mpegpipe` hands over as C422p10, C420p10, ...); the output has
the input's format.  N_FRAMES must be 2, as for the PNG tool.  --flow_scale 2|4 runs the two U-Nets at 1/2 or 1/4 of the frame size and synthesises at full size (the frame is
then padded to x64 / x128): several times faster on UHD material, an approximation of the default output, not parity with the reference.
--tile HxW runs the frame in overlapping windows of tile + halo and stitches them with a cross-fade (--halo, --blend): the activations
are those of a window instead of the frame, which is what lets 8K material, or 4K on a card shared with other work, run at all; likewise
an approximation of the default output, not parity.

--fps N[:D] and --speed X leave the fixed grid: the output follows ssm_amd.video.Timeline, one frame every speed * input rate / fps input
frames (24 -> 60, 25 -> 60, 23.976 -> 59.94 as --fps 60000:1001, 29.97 -> 25, --speed 0.3 or 3/10 for slow motion that is no integer
factor).  --fps alone is speed 1, --speed alone keeps the input's rate in the header.  A frame that falls on an input frame is that
frame's own bytes; pairs that get no frame are not run.  Neither goes together with --upsample_rate or --slowmo.

--shutter DEG [--shutter_samples S], with --fps or --speed: every output frame is the mean of S sub-frames (default 8, a convention) spread
over the first DEG / 360 of its interval, as a camera at the output rate with that shutter angle would have blurred it - 60 -> 24 with
--shutter 180 instead of dropped frames that strobe, slow motion with a chosen amount of blur, or blurred / sharp frame pairs from
high-rate footage.  Every output frame then comes from the GPU, input frames are no longer passed through.  The header's rate is what it
is without --shutter.  --shutter_light coded|bt709|srgb|bt1886|pq|hlg says of what the mean is taken: of the gamma-coded R'G'B' values, as a
frame-mixing filter does (coded, the default), or of the light they stand for under that curve, which is what a sensor integrates - the
mean of codes 0 and 255 is 128 on the codes and 188 in light under sRGB, so streaks of bright objects over a dark ground keep their
brightness.  Which curve a clip wants depends on how it was graded (bt709: camera-referred material; srgb, bt1886: material mastered on a
display); no Y4M header says, so the choice is yours.  Values the network synthesises outside [0, 1] are clipped before they count as
light.  The curve acts on R'G'B' after the matrix and is independent of --matrix and --range.  --shutter_light pq|hlg are the transfer
functions of HDR clips (BT.2100; what phones and cameras record as 10-bit HLG, and graded HDR masters as PQ, usually with --matrix
bt2020): pq is the PQ EOTF, display light up to 10000 cd/m2, hlg the inverse of the HLG OETF, scene light; no OOTF is applied to either.
The coded mean darkens a PQ highlight's streak by more than a factor of 20 in cd/m2, where it costs 128 against 188 codes under sRGB.
--shutter_window box|triangle|hann|gauss[:K] gives the S sub-frames their weights: box (the default) weighs them alike, so a fast object
is S evenly bright copies with hard ends; the others fall off towards the ends of the exposure (ssm_amd.video.shutter_window, sample j at
(j + 1/2) / S of the open interval), and the streak fades in and out at the same S and the same cost.  gauss spans +-K standard
deviations, K = 2 unless given (a convention).  It goes with every --shutter_light; --log names the window, its weights and its scale.

--scene_cut T (a decimal or a fraction in (0, 1]; no default value - the option is off unless given): every pair of input frames is also
scored by ssm_amd.video.SceneCuts from the sum of its absolute luma differences (taken on the GPU, beside the pair's own work), and a pair
that scores T or more is a scene cut: instead of frames that morph one scene into the other, the output repeats the left input frame up
to the middle of the interval and the right one from there on.  The score - the mean absolute luma difference, damped by its own change
from the pair before, over 255 - is a convention, not backed by a measurement here; every cut is written to --log with its score, which
is what to choose T from.  Fades and dissolves are not looked for.  Not together with --shutter, and for 8-bit input only.

--deinterlace auto|tff|bff: the input is interlaced (1080i50, 576i50, ...; `It` / `Ib` in the header), and its n frames come out as 2n
progressive frames at twice the rate.  Every output frame has one field's lines as their own bytes; the lines between them are the field
the network synthesises at t = 1/2 between the field before and the field after, which were sampled at those very line positions (the
clip's first and last output have no such neighbour and get line averages).  auto takes the field order from the header and refuses a
header that does not name one; tff / bff say it (ffmpeg writes `Ip` for interlaced material whose order it does not know).  It goes with
--matrix, --range, --flow_scale and --tile, not with --upsample_rate, --slowmo, --fps, --speed, --shutter or --scene_cut: to retime as
well, chain two runs,  ... --deinterlace auto --output - | interpolate_video.py ... --input - --fps 60 .

--detelecine: the input is film carried in 29.97 frames/s video by 3:2 pulldown (DVDs, NTSC broadcast masters, archive transfers), and the
pulldown is undone before anything else: the cadence is found from the differences of same-parity fields of neighbouring frames (summed on
the GPU, ssm_field_diff_fwd), per window of five frames the frame that holds nothing new is dropped and the two split fields are paired
again.  What follows sees the film's own frames, byte for byte, as a progressive clip at 4/5 of the rate (30000:1001 -> 24000:1001), so it
goes with every option but --deinterlace and --field_probe: --detelecine --fps 60000:1001 is 24 -> 60 without the 2-3 judder.  The field order falls out of
the data: It, Ib, Ip and I? headers are all taken.  There is no threshold; the windows whose cadence changed go to --log with their best
and second-best score.  2:2 and mixed cadences, soft telecine and the orphan field at an edit inside a cycle are out of scope.

--dedup [HI:LO:FRAC] [--dedup_max D]: the input holds frames that repeat the one before - animation drawn on twos or threes, 24 or 25
frames/s brought to 50 or 60 by repetition, screen recordings, captures that filled a dropped frame with a copy - and runs of up to D
(default 2) such frames are repaired: the output keeps the grid of --upsample_rate (frame count and rate are what they are without the
option), but the places of the repeats, and of everything between the run's two neighbours, are filled by frames synthesised between
those two, so slow motion of such a clip no longer stutters as its source did.  --upsample_rate 1 is legal here and means repair only.
A frame is a repeat when, in every plane, no 8 x 8 block differs from the frame before by more than HI in its sum of absolute
differences, and at most the fraction FRAC of the blocks by more than LO (summed on the GPU, ssm_block_sad_fwd, a chunk ahead of the
loop).  The defaults, 768:320:0.33 scaled to the clip's bit depth, are the numbers of ffmpeg's mpdecimate, not its construction, and
not measured on compressed footage: a convention; 0:0:0 takes exact repeats only.  A longer run is a still and a run at the clip's end
has no right neighbour: both stay as they are.  Every run goes to --log with its length, whether it was repaired, and its worst block
sum and count.  It goes with --slowmo, --matrix, --range, --flow_scale, --tile and --detelecine (which runs first), not with --fps,
--speed, --shutter, --scene_cut or --deinterlace: chain two runs,  ... --dedup --upsample_rate 1 --output - | interpolate_video.py ... .

--active auto[:LIM[:FRAC]] | W:H:X:Y [--active_probe P]: the input is letterboxed or pillarboxed (a 2.39:1 picture in a 1920x1080 frame),
and the run is that of the picture alone: the rectangle is cut out of every frame on the GPU, the network runs on the canvas of the
cropped clip (804 rows pad to 832, not to 1088), and each synthesised picture is pasted into the bars of the nearer input frame - the
left one before the middle of the interval, the right one from there on.  The bars of every output frame are then some input frame's own
bytes: their edge no longer pulses between clean input frames and synthesised ones, and a subtitle or a logo in a bar steps with its
own frames instead of being warped.  Input frames pass through whole, as ever.  W:H:X:Y is the order `ffmpeg -vf cropdetect` prints, so
its crop=... can be pasted; it has to sit on the chroma grid (even X, W, and in 4:2:0 even Y, H, or the frame's edge).  auto finds the
smallest such rectangle that holds every active row and column of the first P frames (default 48): a luma sample counts when it is above
LIM (default 24 at 8 bits, scaled to the depth), a row or column is active when more than FRAC (default 1/64) of its samples count
(counted on the GPU, ssm_luma_counts_fwd).  24 is the number of cropdetect's limit, not its construction, and 1/64 is this tool's own:
conventions, not measured on compressed footage, whose bars are noisy.  If the rectangle is the whole frame, nothing is active, or it is
under 32 samples in a direction, the run is the one without the option, byte for byte, and --log says so.  A later frame with active
lines outside the rectangle goes to --log and changes nothing: a rectangle that changes inside a clip, coloured bars and re-planning are
out of scope.  It goes with --upsample_rate, --slowmo, --fps, --speed, --scene_cut, --matrix (whose default stays that of the FRAME's
height), --range, --flow_scale, --tile and --detelecine (which runs first), not with --shutter, --deinterlace or --dedup: chain two runs.

--field_probe [P]: the field order is looked for in the data.  `ffmpeg -f yuv4mpegpipe` writes `Ip` for interlaced material whose order it
does not know, and nothing refuses a wrong tff / bff: the fields are then woven in the wrong temporal order and every second output steps
back in time.  Per frame of the first P (default 48) the luma rows are compared with the mean of their two neighbours, in the frame
before, the frame after and the frame itself (three exact sums A0, A1, D on the GPU, ssm_field_order_sums_fwd); a frame is top field
first when 25 A0 > 26 A1, bottom field first when 25 A1 > 26 A0, progressive in motion when twice the smaller exceeds 3 D, else
undetermined, and the verdict is the kind of more than half of the determined frames (ssm_amd.video.FieldVerdict).  With --deinterlace
auto and a header that says Ip or I? the verdict is the run's field order; a verdict of progressive or none is refused before anything is
written, with the four counts, and asks for tff or bff.  With an It / Ib header, and with --deinterlace tff|bff, the order is what it is
without the option and a verdict that contradicts it is a warning in --log that changes nothing.  Without --deinterlace it is a report:
the clip runs as it does without the option, and a clip that looks interlaced gets one line in --log that names --deinterlace tff|bff.
The ratios 26/25 and 3/2 are conventions in the spirit of ffmpeg's idet, not its construction - nothing claims its decisions frame for
frame, ffmpeg is not compared - and not measured on noisy or compressed footage; a hard-edged shape that moves by whole rows can read as
bottom field first.  Frames behind the probe are not watched; Im, a per-frame order and chroma are out of scope.  Not with --detelecine
(a telecined clip is a mixture by construction) or a recurrent model.

--static LO: blocks that do not change keep their bytes.  A channel logo over moving picture, burnt-in subtitles or a timecode, the static
parts of a screen recording or of animation and a locked-off background are the same samples in both input frames of a pair, yet they
come out of the network re-quantised and pulled by the flow of what moves beside them, and every upsample_rate-th output is an input
frame's own bytes: such areas pulse.  With the option, where the two frames of a pair agree on an 8 x 8 block - the sum of absolute
differences over its luma and the chroma under it is at most LO, in codes of the clip's depth - every frame between them carries the left
frame's samples of that block (decided and pasted on the GPU, ssm_static_paste_fwd, behind the colour conversion of every pass).
--static 0 is exact, not a heuristic: both neighbours hold those samples, and no honest in-between frame differs there.  Any other LO is
your number: there is no default, and the 320 at 8 bits that mpdecimate's lo would suggest is not backed by any measurement.  A block
that agrees in both frames while something crossed it in between is kept (nothing can tell), and the seams between kept and synthesised
blocks are not smoothed.  --log gets one line with the pairs, the blocks kept of all and the largest and smallest share, and one line for
every pair without a static block when others had some.  It goes with --upsample_rate, --slowmo, --fps, --speed, --scene_cut (a cut
pair's frames are replaced whole, as without it), --matrix, --range, --flow_scale, --tile and --detelecine (which runs first), and with
every format; not with --shutter (every output comes from the accumulator), --deinterlace, --dedup or --active: chain two runs.

--flow_check [T[:ALPHA:BETA]]: the network's own opinion of its flows.  Stage 1 estimates the motion 0 -> 1 and the motion 1 -> 0
independently; where following one and then the other does not lead back, the pixel is occluded or a flow is wrong - where interpolated
footage tears and ghosts.  Every pass scores that on the GPU (ssm_flow_consistency_fwd on the two fields where stage 1 left them; the
definition stands in include/ssm_hip.h): a pixel is inconsistent when |F + G'|^2 > ALPHA (|F|^2 + |G'|^2) + BETA, a pair's score is the
larger share of inconsistent pixels of its two directions.  --log gets one line with the pairs scored, the least, median and largest
score and the largest mean residual.  With T a pair whose score reaches T gets the nearer input frame's bytes instead of its synthesised
frames, the rule of --scene_cut, and a line in --log.  ALPHA:BETA default to 0.01:0.5, the numbers of Sundaram, Brox and Keutzer (2010)
as most later work uses them: a convention, not backed by a measurement here; there is no default T, and with the synthetic weights of
this repository a score says nothing about quality.  It goes with --upsample_rate, --slowmo, --fps, --speed, --scene_cut, --static,
--active, --matrix, --range and --detelecine; not with --shutter, --deinterlace, --dedup, --flow_scale other than 1, --tile or a
recurrent model.

--flow_blocks K (with --flow_check): the check's fallback per 8 x 8 block instead of per pair.  The blocks are those of --static.  Where
more than K of a block's 64 luma pixels are inconsistent in at least one direction, every frame synthesised between the pair carries the
NEARER input frame's samples of that block, luma and chroma - the left frame's below t = 1/2, the right one's from there on (decided and
pasted on the GPU, ssm_flow_paste_fwd, behind the colour conversion of every pass and ahead of --static's paste).  K = 64 fails nothing
and is the run without it, byte for byte; K = 0 fails every block with one inconsistent pixel; there is no default K.  --log gets one
line with the pairs, the blocks replaced of all and the largest and smallest share per pair, and one line per pair in which every block
failed.  --flow_check without T and --flow_blocks is the report plus the per-block fallback; with T a pair that reaches it is still
replaced whole.  Not claimed: the seams between pasted and synthesised blocks are not smoothed, a block from the nearer frame inside a
moving region steps rather than moves, and with the synthetic weights of this repository nothing can be said about quality.  Not with
--active: chain two runs.

--flow_fallback nearer|mix (with --flow_blocks): what a failed block carries.  nearer is the rule above and the default.  mix: the
cross-fade of the pair's two frames at the output's exact time, a (1 - t) + b t rounded half up in exact integers (ssm_flow_mix_fwd in
place of ssm_flow_paste_fwd; the definition stands in include/ssm_hip.h) - a failed block inside a moving region then changes with every
output instead of standing still and jumping at t = 1/2.  With --fps / --speed the times are whole numbers over the denominator of the
timeline's step, which may be at most 65535 (24 -> 59.94 gives 2500, 29.97 -> 25 gives 1001); a larger one is refused before anything is
written.  A pair that reaches --flow_check's T, and a cut pair, are still replaced whole by the nearer frame.  Not claimed: where nearer
steps, mix ghosts; which looks better is not known, and cannot be with the synthetic weights of this repository; there is still no
default K; the seams are not smoothed.
"""
import argparse
import configparser
import logging
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from models import superslomo_r as ssm  # noqa: E402
from ssm_amd import flow_eval as FE  # noqa: E402
from ssm_amd import tiles as T  # noqa: E402
from ssm_amd import video as V  # noqa: E402

log = logging.getLogger(__name__)


def _named(parse):
    """An argparse type whose usage error carries the parser's own message, which names the value."""
    def f(text):
        try:
            return parse(text)
        except ValueError as e:
            raise argparse.ArgumentTypeError(str(e)) from None
    return f


def getargs(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("-c", "--config", required=True, default="config.ini", help="Path to config.ini file.")
    parser.add_argument("--expt", required=True, help="Experiment Name.")
    parser.add_argument("--log", required=True, help="Path to logfile.")
    parser.add_argument("--input", required=True, help="Input .y4m file, or - for stdin.")
    parser.add_argument("--output", required=True, help="Output .y4m file, or - for stdout.")
    parser.add_argument("--upsample_rate", type=int, default=None,
                        help="Integer upsampling rate. For 30FPS -> 240FP, use 8. For 1080FPS, use 36. Default 8.")
    parser.add_argument("--fps", type=_named(V.parse_rate), default=None, metavar="N[:D]",
                        help="Output frame rate, written into the header as given (60, 60000:1001): any rate, not only a multiple of the input's.")
    parser.add_argument("--speed", type=_named(V.parse_speed), default=None, metavar="X",
                        help="Playback speed as a decimal or a fraction (0.25, 1/4, 3/10); below 1 is slow motion. Default 1.")
    parser.add_argument("--shutter", type=_named(V.parse_shutter), default=None, metavar="DEG",
                        help="Shutter angle in degrees, above 0 and at most 360 (180, 172.8, 90): every output frame is the mean of sub-frames "
                             "over DEG / 360 of its interval. Needs --fps or --speed. Default: off.")
    parser.add_argument("--shutter_samples", type=int, default=8, metavar="S",
                        help="With --shutter: sub-frames per output frame (a convention, not a measured optimum). Default 8.")
    parser.add_argument("--shutter_light", choices=V.SHUTTER_LIGHTS + V.HDR_LIGHTS, default="coded",
                        help="With --shutter: average the coded values (coded) or the light they stand for under a curve (bt709, srgb, "
                             "bt1886; for HDR clips pq, hlg); which curve fits depends on how the clip was graded. Default coded.")
    parser.add_argument("--shutter_window", type=_named(V.parse_shutter_window), default=V.parse_shutter_window("box"),
                        metavar="box|triangle|hann|gauss[:K]",
                        help="With --shutter: the weights of the sub-frames. box: all alike; triangle, hann, gauss[:K] (+-K standard deviations, "
                             "default 2, a convention) fall off towards the ends of the exposure. Default box.")
    parser.add_argument("--scene_cut", type=_named(V.parse_scene_cut), default=None, metavar="T",
                        help="Scene-cut threshold as a decimal or a fraction in (0, 1] (0.1, 1/10): a pair of input frames whose score reaches it "
                             "gets copies of its input frames instead of synthesised ones. A convention, no measured optimum; no default "
                             "value: off unless given. Not together with --shutter.")
    parser.add_argument("--matrix", choices=sorted(V.MATRICES), default=None, help="Y'CbCr matrix (default: bt709 from 720 rows up, else bt601; bt2020, non-constant luminance, only when asked for).")
    parser.add_argument("--range", choices=sorted(V.RANGES), default=None, dest="color_range",
                        help="Code range (default: the header's XCOLORRANGE tag, else limited).")
    parser.add_argument("--slowmo", action="store_true", help="Keep the input's frame rate in the output header: slow motion.")
    parser.add_argument("--flow_scale", type=int, choices=(1, 2, 4), default=1,
                        help="Coarse-flow mode: run both U-Nets at 1/flow_scale of the frame size and synthesise at full size (faster on HD and "
                             "UHD material; an approximation of the default output, not parity). Default 1: off.")
    parser.add_argument("--tile", type=T.parse_tile, default=None, metavar="HxW",
                        help="Tiled mode: run the frame in overlapping windows with cores of H x W pixels (multiples of 32) and stitch them "
                             "(less memory; an approximation of the default output, not parity). Default: off.")
    parser.add_argument("--halo", type=int, default=T.DEFAULT_HALO, help="With --tile: pixels of context around a tile's core (multiple of 32).")
    parser.add_argument("--blend", type=int, default=T.DEFAULT_BLEND,
                        help="With --tile: half width of the cross-fade over a seam (0 or a power of two >= 4, at most the halo).")
    parser.add_argument("--deinterlace", choices=V.DEINTERLACE, default=None,
                        help="The input is interlaced: write its 2n fields as progressive frames at twice the rate, the missing lines "
                             "synthesised from the neighbouring fields. auto: the field order of the header; tff, bff: as said. Default: off.")
    parser.add_argument("--detelecine", action="store_true",
                        help="The input is film in 3:2 pulldown: find the cadence, drop the repeated fields and pair the split ones again "
                             "before anything else; the clip then runs as progressive at 4/5 of its rate. Not together with --deinterlace.")
    parser.add_argument("--dedup", type=_named(V.parse_dedup), nargs="?", const=True, default=None, metavar="HI:LO:FRAC",
                        help="Repair runs of frames that repeat the one before: their places are filled by frames synthesised between the "
                             "run's neighbours. HI:LO:FRAC: per plane no 8x8 block sum of absolute differences above HI and at most FRAC of "
                             "the blocks above LO; default 768:320:0.33 at 8 bits (a convention), 0:0:0 exact repeats only. Default: off.")
    parser.add_argument("--dedup_max", type=_named(V.parse_dedup_max_text), default=V.DEDUP_MAX, metavar="D",
                        help="With --dedup: the longest run of repeats that is repaired; longer runs are stills and stay. Default 2.")
    parser.add_argument("--active", type=_named(V.parse_active), default=None, metavar="auto[:LIM[:FRAC]]|W:H:X:Y",
                        help="The input is letterboxed: run on the picture alone and keep the bars of the nearer input frame. auto finds the "
                             "rectangle from the first --active_probe frames (luma above LIM, default 24 at 8 bits, in more than FRAC, default "
                             "1/64, of a line: conventions); W:H:X:Y gives it, in the order ffmpeg's cropdetect prints. Default: off.")
    parser.add_argument("--active_probe", type=_named(V.parse_active_probe), default=V.ACTIVE_PROBE, metavar="P",
                        help="With --active auto: the frames the rectangle is decided on. Default 48.")
    parser.add_argument("--field_probe", type=_named(V.parse_field_probe), nargs="?", const=V.FIELD_PROBE, default=None, metavar="P",
                        help="Look for the field order in the first P frames (default 48; comb sums on the GPU). With --deinterlace auto and a "
                             "header that says Ip or I? the verdict is the run's order; else a warning or a report. Default: off.")
    parser.add_argument("--static", type=_named(V.parse_static), default=None, metavar="LO",
                        help="Blocks that do not change keep their bytes: where the two frames of a pair differ by at most LO in the sum of "
                             "absolute differences over an 8x8 block (luma and the chroma under it), the frames between them carry the left "
                             "frame's samples. 0: only blocks that are the same in both, exact. No default value: off unless given.")
    parser.add_argument("--flow_check", type=_named(FE.parse_flow_check), nargs="?", const=(None, None, None), default=None,
                        metavar="T[:ALPHA:BETA]",
                        help="Score every pair's two flows against each other on the GPU (forward-backward consistency) and log the scores. "
                             "With T, a decimal or a fraction: a pair whose share of inconsistent pixels reaches T gets copies of its input "
                             "frames, like a scene cut. ALPHA:BETA default to 0.01:0.5, a convention of the literature; no default T.")
    parser.add_argument("--flow_blocks", type=_named(lambda text: V.parse_flow_blocks(text, "--flow_blocks")), default=None, metavar="K",
                        help="With --flow_check: fall back per 8x8 block instead of per pair. A block of a synthesised frame in which more "
                             "than K of the 64 luma pixels are inconsistent in at least one direction takes the nearer input frame's "
                             "samples. 0 .. 64; 64 changes nothing. No default value: off unless given. Not together with --active.")
    parser.add_argument("--flow_fallback", type=_named(lambda text: V.parse_flow_fallback(text, "--flow_fallback")), default="nearer",
                        metavar="nearer|mix",
                        help="With --flow_blocks: what a failed block takes. nearer: the nearer input frame's samples. mix: the cross-fade "
                             "of the two input frames at the output's exact time, rounded half up, on the GPU. Default: nearer.")
    args = parser.parse_args(argv)
    refusal = V.flag_refusal(dict(vars(args), target_rate=args.fps,
                                  shutter_window=None if args.shutter_window[0] == "box" else V.window_name(args.shutter_window)))
    if refusal is not None:
        parser.error(refusal)
    if args.flow_blocks is not None and args.flow_check is None:          # a sub-option of --flow_check: after the table has spoken
        parser.error("--flow_blocks is --flow_check's per-block fallback: it needs --flow_check")
    if args.flow_blocks is not None and args.active is not None:
        parser.error("--flow_blocks does not go together with --active: the blocks of the per-block fallback are the whole frame's, not a "
                     "cut window's; chain two runs")
    if args.flow_fallback != "nearer" and args.flow_blocks is None:          # a sub-option of --flow_blocks
        parser.error("--flow_fallback %s is what a failed block of --flow_blocks carries: it needs --flow_blocks" % args.flow_fallback)
    if args.dedup is not None and args.upsample_rate is not None and args.upsample_rate < 1:
        parser.error("--upsample_rate must be at least 1 with --dedup (got %d)" % args.upsample_rate)
    if args.shutter is not None and args.shutter_samples < 1:
        parser.error("--shutter_samples must be at least 1 (got %d)" % args.shutter_samples)
    if args.upsample_rate is None and args.fps is None and args.speed is None and args.deinterlace is None:
        args.upsample_rate = 8
    return args


def static_lines(static, lo):
    """What --log gets of a run with --static: `static` = [(i, static blocks, blocks)] of the pairs that got outputs.  One summary line,
    and one line for every pair without a static block when others had some."""
    if not static:
        return ["static: lo = %d, no pair got a synthesised frame" % lo]
    kept, of = sum(s for _, s, _ in static), sum(b for _, _, b in static)
    if of == 0:
        return ["static: lo = %d, %d pairs, the frame has no 8 x 8 block: nothing is kept" % (lo, len(static))]
    shares = [s / b for _, s, b in static]
    lines = ["static: lo = %d, %d pairs, %d of %d blocks kept (%.2f%%), per pair at most %.2f%% and at least %.2f%%"
             % (lo, len(static), kept, of, 100.0 * kept / of, 100.0 * max(shares), 100.0 * min(shares))]
    if kept:
        lines += ["static: no static block between input frames %d and %d" % (i, i + 1) for i, s, _ in static if s == 0]
    return lines


def flow_check_lines(checks, failed, option):
    """What --log gets of a run with --flow_check: `checks` = [(i, FlowCheck)] of the pairs that ran, `failed` those that reached the
    threshold, option = (T or None, alpha, beta).  One summary line - the pairs scored, the least, median and largest score, the largest
    mean residual - and one line per failed pair."""
    t, alpha, beta = option
    head = "flow check: alpha = %g, beta = %g%s" % (alpha, beta, "" if t is None else ", threshold %s" % t)
    if not checks:
        return [head + ", no pair ran"]
    scores = sorted(c.score for _, c in checks)
    lines = [head + ", %d pairs scored: score at least %.6f, median %.6f, at most %.6f; largest mean residual %.4f px%s"
             % (len(checks), float(scores[0]), float(scores[(len(scores) - 1) // 2]), float(scores[-1]),
                max(c.mean_residual for _, c in checks), "" if t is None else "; %d pairs fell back to input frames" % len(failed))]
    lines += ["flow check failed between input frames %d and %d: score %s = %.6f (threshold %s), mean residual %.4f px"
              % (i, i + 1, c.score, float(c.score), t, c.mean_residual) for i, c in failed]
    return lines


def flow_blocks_lines(repaired, k, fallback="nearer"):
    """What --log gets of a run with --flow_blocks: `repaired` = [(i, failed blocks, blocks)] of the pairs that got outputs.  One summary
    line, which names a --flow_fallback other than nearer, and one line for every pair in which every block failed."""
    head = "flow blocks: K = %d" % k + ("" if fallback == "nearer" else ", fallback %s" % fallback)
    if not repaired:
        return [head + ", no pair got a synthesised frame"]
    failed, of = sum(f for _, f, _ in repaired), sum(b for _, _, b in repaired)
    if of == 0:
        return [head + ", %d pairs, the frame has no 8 x 8 block: nothing is replaced" % len(repaired)]
    shares = [f / b for _, f, b in repaired]
    lines = [head + ", %d pairs, %d of %d blocks replaced (%.2f%%), per pair at most %.2f%% and at least %.2f%%"
             % (len(repaired), failed, of, 100.0 * failed / of, 100.0 * max(shares), 100.0 * min(shares))]
    lines += ["flow blocks: every block failed between input frames %d and %d" % (i, i + 1) for i, f, b in repaired if f == b]
    return lines


def main(argv=None, model=None):
    args = getargs(argv)
    config = configparser.RawConfigParser()
    logging.basicConfig(filename=args.log, level=logging.INFO)
    if not config.read(args.config):
        raise FileNotFoundError(args.config)
    matrix = None if args.matrix is None else V.MATRICES[args.matrix]
    crange = None if args.color_range is None else V.RANGES[args.color_range]
    model = (model if model is not None else ssm.FullModel(config)).cuda().eval()
    timed = args.fps is not None or args.speed is not None
    vi = V.VideoInterpolator(model, config, upsample_rate=args.upsample_rate, matrix=matrix, color_range=crange,
                             flow_scale=args.flow_scale, tile=args.tile, halo=args.halo, blend=args.blend, target_rate=args.fps, speed=args.speed,
                             shutter=args.shutter, shutter_samples=args.shutter_samples, scene_cut=args.scene_cut,
                             shutter_light=args.shutter_light, shutter_window=args.shutter_window, deinterlace=args.deinterlace, dedup=args.dedup, dedup_max=args.dedup_max,
                             active=args.active, active_probe=args.active_probe, field_probe=args.field_probe, static=args.static,
                             flow_check=None if args.flow_check is None else (True if args.flow_check[0] is None else args.flow_check[0]),
                             flow_alpha=args.flow_check and args.flow_check[1], flow_beta=args.flow_check and args.flow_check[2],
                             flow_blocks=args.flow_blocks, flow_fallback=args.flow_fallback)
    with V.Y4MReader(args.input, extended=True, interlaced=args.deinterlace is not None or args.detelecine) as reader:
        if args.detelecine:
            log.info("[%s] detelecine: %d:%d frames/s in, film at %d:%d", args.expt, *reader.rate, *V.detelecine_rate(reader.rate))
            reader = V.TelecineSource(reader, next(model.parameters()).device)
        if args.field_probe is not None:          # ahead of the writer: a refused verdict leaves no output behind
            reader = vi.probe_fields(reader)
            log.info("[%s] %s", args.expt, vi.field_probe.note)
            if vi.field_probe.warning is not None:
                log.warning("[%s] %s", args.expt, vi.field_probe.warning)
            if vi.field_probe.advice is not None:
                log.info("[%s] %s", args.expt, vi.field_probe.advice)
        if args.deinterlace is not None:
            rate = V.output_rate(reader.rate, 2)
            order = vi.field_probe.order if args.field_probe is not None else V.field_order(args.deinterlace, reader.interlace)
            log.info("[%s] deinterlace: %s, fields as frames", args.expt, order)
        elif timed:
            rate = args.fps or reader.rate
            tl = vi.timeline(reader.rate)
            log.info("[%s] timeline: step = %s input frames per output frame, slots = %d times per pair", args.expt, tl.step, tl.slots)
            if tl.samples > 1:
                log.info("[%s] shutter: %s of the interval in %d samples, averaged in %s", args.expt, tl.shutter, tl.samples,
                         "coded values" if args.shutter_light == "coded" else "light (%s)" % args.shutter_light)
                w, scale = V.shutter_window(args.shutter_window, tl.samples)
                log.info("[%s] shutter window: %s, weights %s, scale %.9g%s", args.expt, V.window_name(args.shutter_window),
                         " ".join("%.9g" % x for x in w), scale,
                         " (the unweighted calls)" if args.shutter_window[0] == "box" else "")
        else:
            rate = V.output_rate(reader.rate, args.upsample_rate, args.slowmo)
            if args.dedup is not None:
                log.info("[%s] dedup: hi:lo:frac = %s:%s:%s, runs of up to %d repeats are repaired, slots = %d times per pair", args.expt,
                         *V.dedup_thresholds(args.dedup, getattr(reader, "bits", 8)), args.dedup_max, vi.gap_timeline().slots)
        out_range = crange if crange is not None else (reader.color_range if reader.color_range is not None else V.LIMITED)
        log.info("[%s] %s: %dx%d C%s at %d:%d frames/s -> %s at %d:%d", args.expt, args.input, reader.width, reader.height, reader.chroma,
                 reader.rate[0], reader.rate[1], args.output, rate[0], rate[1])
        with V.Y4MWriter.like(args.output, reader, rate=rate, color_range=out_range) as writer:
            n = vi.run(reader, writer)
    if args.detelecine:
        if reader.combed_first:
            log.info("[%s] detelecine: frame 0 sits at cadence position 3 and has no predecessor: written as it stands", args.expt)
        last = None
        for first, h, best, second in reader.cadence:
            if h != last:
                log.info("[%s] detelecine: from input frame %d cadence h = %d (%s field first, phase %d): score %d, second best %d", args.expt,
                         0 if last is None else first, h, "bottom" if h >= 5 else "top", h % 5, best, second)
            last = h
        log.info("[%s] detelecine: %d windows, %d input frames dropped", args.expt, len(reader.cadence), reader.dropped)
    for first, m, repaired, worst_max, worst_over in vi.repeats:
        log.info("[%s] dedup: %d repeat%s from input frame %d: %s; worst block sum %d, most blocks over lo %d", args.expt, m, "" if m == 1 else "s",
                 first, "repaired" if repaired else "left as they are (%s)" % ("a still" if m > args.dedup_max else "the clip ends"), worst_max,
                 worst_over)
    if args.dedup is not None:
        log.info("[%s] dedup: %d runs, %d repaired", args.expt, len(vi.repeats), sum(1 for r in vi.repeats if r[2]))
    if args.active is not None:
        log.info("[%s] active: %s%s", args.expt, vi.active_note, "" if vi.active is not None else "; the run is whole-frame, as without --active")
        for i, rows, cols in vi.active_excess:
            log.info("[%s] active: input frame %d has %d active rows and %d active columns outside the rectangle; nothing changes", args.expt, i,
                     rows, cols)
    if args.static is not None:
        for line in static_lines(vi.static, args.static):
            log.info("[%s] %s", args.expt, line)
    if args.flow_check is not None:
        for line in flow_check_lines(vi.flow_checks, vi.flow_failed, vi.flow_check):
            log.info("[%s] %s", args.expt, line)
    if args.flow_blocks is not None:
        for line in flow_blocks_lines(vi.flow_repaired, args.flow_blocks, args.flow_fallback):
            log.info("[%s] %s", args.expt, line)
    for i, score in vi.cuts:
        log.info("[%s] scene cut between input frames %d and %d: score %s = %.6f (threshold %s)", args.expt, i, i + 1, score, float(score),
                 vi.scene_cut)
    log.info("Interpolation complete: %d frames written.", n)
    return n


if __name__ == "__main__":
    main()
