#!/usr/bin/env python3
"""Score a clip against its own held-out frames, streamed: a YUV4MPEG2 (.y4m) file or pipe of HIGH-RATE footage in, a table of PSNR out.

    ffmpeg -i gopro240.mp4 -f yuv4mpegpipe - | evaluate_video.py -c cfg.ini --expt e --log run.log --input - --hold 8

Every --hold-th frame of the input is kept, the frames in between are synthesised exactly as `interpolate_video.py --upsample_rate HOLD`
would synthesise them from the kept frames alone, and each is compared with the real frame that was left out: the sum of squared
differences of the Y, U and V samples as the tool would write them, taken on the GPU (ssm_plane_sse_fwd) beside the pair's own work.  This
is the procedure of evaluate_interpolation_results.py on Adobe240, on the streamed loop: at the tool's rate, for every format the tool
reads (4:2:0, 4:2:2, 4:4:4, 8 to 16 bits) and for --flow_scale and --tile, in memory that does not depend on the clip's length.

Beside the model's score stands `nearest`: the held-out frame against the nearer of its two kept neighbours, the do-nothing baseline.  A
model that does not beat it on a clip is not interpolating.  PSNR is 10 log10(peak^2 / MSE) with peak = 2^bits - 1 whatever the code
range, the convention of `ffmpeg -lavfi psnr`; frames and planes are pooled by their sums of squares, never by their dB.  The frames after
the last kept one ((n - 1) mod HOLD of them) are read and not scored; their number is reported.

--mix adds the baseline an interpolator really has to beat: the held-out frame against the cross-fade of its two kept frames at k / HOLD,
which is what frame blending and every cheap rate converter writes (ssm_payload_mix_fwd, on the GPU).  --ssim adds, for every column, the
SSIM of x264 and of ffmpeg's `ssim` filter (8 x 8 windows at stride 4, per plane; ssm_plane_ssim_fwd), pooled over frames and planes by
window counts - `avg` is therefore not ffmpeg's plane-size weighted "All".  Both append to the table and to the --stats lines; without
them the report is unchanged.

--stats FILE writes one line per scored frame (n: the input frame's index, k: its place between the kept frames, t = k / HOLD), in the
manner of the psnr filter's stats_file.  --output FILE writes the clip that interpolate_video.py would write for the decimated input:
kept frames as their own bytes, synthesised frames between, at the input's rate.  The summary goes to --log and to stdout.

With the synthetic weights of this repository's tests the numbers say nothing about quality; they show that the instrument works.
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
from ssm_amd import tiles as T  # noqa: E402
from ssm_amd import video as V  # noqa: E402
from ssm_amd import video_score as VS  # noqa: E402

log = logging.getLogger(__name__)


def _hold(text):
    try:
        hold = int(text)
        VS.hold_out_plan(0, hold)
    except ValueError:
        raise argparse.ArgumentTypeError("hold must be a whole number, at least 2 (got %r)" % (text,)) from None
    return hold


def getargs(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("-c", "--config", required=True, default="config.ini", help="Path to config.ini file.")
    parser.add_argument("--expt", required=True, help="Experiment Name.")
    parser.add_argument("--log", required=True, help="Path to logfile.")
    parser.add_argument("--input", required=True, help="Input .y4m file of high-rate footage, or - for stdin.")
    parser.add_argument("--hold", required=True, type=_hold, metavar="N",
                        help="Keep every N-th frame and score the N - 1 frames synthesised between two kept ones against the frames left out.")
    parser.add_argument("--stats", default=None, metavar="FILE", help="Write one line per scored frame to FILE.")
    parser.add_argument("--ssim", action="store_true", help="Also report SSIM (8 x 8 windows at stride 4, per plane) for every column.")
    parser.add_argument("--mix", action="store_true",
                        help="Also score the cross-fade of the two kept frames against the held-out frame: the frame-blending baseline.")
    parser.add_argument("--output", default=None, help="Also write the interpolated decimated clip as .y4m (- for stdout). Default: frames are dropped.")
    parser.add_argument("--matrix", choices=sorted(V.MATRICES), default=None, help="Y'CbCr matrix (default: bt709 from 720 rows up, else bt601; bt2020, non-constant luminance, only when asked for).")
    parser.add_argument("--range", choices=sorted(V.RANGES), default=None, dest="color_range",
                        help="Code range (default: the header's XCOLORRANGE tag, else limited).")
    parser.add_argument("--flow_scale", type=int, choices=(1, 2, 4), default=1,
                        help="Score the coarse-flow mode: both U-Nets at 1/flow_scale of the frame size. Default 1: off.")
    parser.add_argument("--tile", type=T.parse_tile, default=None, metavar="HxW",
                        help="Score the tiled mode: overlapping windows with cores of H x W pixels (multiples of 32). Default: off.")
    parser.add_argument("--halo", type=int, default=T.DEFAULT_HALO, help="With --tile: pixels of context around a tile's core (multiple of 32).")
    parser.add_argument("--blend", type=int, default=T.DEFAULT_BLEND,
                        help="With --tile: half width of the cross-fade over a seam (0 or a power of two >= 4, at most the halo).")
    args = parser.parse_args(argv)
    if args.output == "-" and args.stats == "-":
        parser.error("--output - and --stats - both write to stdout: give one of them a file")
    return args


def main(argv=None, model=None):
    """Returns the HoldOutResult."""
    args = getargs(argv)
    config = configparser.RawConfigParser()
    logging.basicConfig(filename=args.log, level=logging.INFO)
    if not config.read(args.config):
        raise FileNotFoundError(args.config)
    matrix = None if args.matrix is None else V.MATRICES[args.matrix]
    crange = None if args.color_range is None else V.RANGES[args.color_range]
    model = (model if model is not None else ssm.FullModel(config)).cuda().eval()
    scorer = VS.HoldOutScorer(model, config, args.hold, matrix=matrix, color_range=crange, flow_scale=args.flow_scale, tile=args.tile,
                              halo=args.halo, blend=args.blend, ssim=args.ssim, mix=args.mix)
    with V.Y4MReader(args.input, extended=True) as reader:
        out_range = crange if crange is not None else (reader.color_range if reader.color_range is not None else V.LIMITED)
        log.info("[%s] %s: %dx%d C%s at %d:%d frames/s, hold = %d -> %s", args.expt, args.input, reader.width, reader.height, reader.chroma,
                 reader.rate[0], reader.rate[1], args.hold, args.output or "no output")
        if args.output is None:
            res = scorer.run(reader)
        else:
            with V.Y4MWriter.like(args.output, reader, color_range=out_range) as writer:
                res = scorer.run(reader, writer)
    if args.stats is not None:
        text = "".join(line + "\n" for line in res.stats_lines())
        if args.stats == "-":
            sys.stdout.write(text)
        else:
            with open(args.stats, "w") as f:
                f.write(text)
    table = res.table()
    for line in table.split("\n"):
        log.info("[%s] %s", args.expt, line)
    (sys.stderr if args.output == "-" else sys.stdout).write(table + "\n")
    log.info("Evaluation complete: %d frames read, %d scored.", res.frames_read, res.scored)
    return res


if __name__ == "__main__":
    main()
