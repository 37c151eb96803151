"""Interlaced clips of the streamed video path (ssm_amd/video.py) on synthetic frames.  Driver, timers and model are
tools/video_bench.py's: three steps, each a child process under its own `timeout`, chained - the first one that fails (or runs into its
limit) ends the run.  Each step prints one JSON line:
  kernel_420jpeg, kernel_422p10
           event-timed ssm_fields_split_fwd (7 frames -> 14 fields) and ssm_fields_weave_fwd (7 kept and 7 synthesised fields -> 7 frames;
           and fill = 1: 7 kept fields -> 7 frames with line averages) at 720 x 1280, beside a device-to-device copy of the same 7
           frame_bytes, ALTERNATED in one run: a round times every call once, window after window.  Per call: the median over `--windows`
           rounds of `--iters` back-to-back calls, with the least and the largest; the call's one-touch bytes (read + written, every byte
           once) as a fraction of the 6.29 TB/s copy ceiling (tools/bench_video.py).  The results are checked against the yardsticks first.
  fps      output frames per second of wall time, file to /dev/null, in turns on the same two HIP streams: VideoInterpolator(deinterlace=
           "auto") on a 64-frame 720 x 1280 `It` clip (128 outputs, 126 pairs of 360 x 1280 fields) beside THIS COMMIT'S OWN
           VideoInterpolator(upsample_rate=2) on a progressive 360 x 1280 clip of 128 frames (255 outputs, 127 pairs of the same size): the
           same work per pair, without split and weave; 2 streams x 1 pair.  Compare per PAIR: pairs_per_s.
Nothing is asserted on the numbers.  With synthetic weights nothing can be said about quality.
Usage: python tools/bench_fields.py [--out profiles/fields_bench.txt] [--only STEP] [--iters 20] [--windows 7] [--runs 3]"""
import os
import statistics
import sys
import tempfile
import time

from video_bench import (COPY_CEILING_BYTES_PER_S, alternated_ms, drive, parser, per_s, run_only, share_streams, synthetic_model, timed_legs,
                         write_y4m)

STEPS = (("kernel_420jpeg", 180), ("kernel_422p10", 180), ("fps", 600))          # step, its time limit in seconds
H, W, CLIP_FRAMES = 720, 1280, 64


def bench_kernel(dev, tag, iters, windows):
    import numpy as np
    import torch
    from ssm_amd import video as V
    n = 7
    layout, bits = V.EXTENDED_TAGS[tag]
    fb = V.frame_bytes(H, W, layout, bits)
    gen = torch.Generator(device="cpu").manual_seed(1)
    host = torch.randint(0, 256, (n, fb), generator=gen, dtype=torch.uint8)
    frames = host.to(dev)
    fields = torch.empty(2 * n, fb // 2, dtype=torch.uint8, device=dev)
    woven = torch.empty(n, fb, dtype=torch.uint8, device=dev)
    V.fields_split(frames, H, W, layout, bits, out=fields)
    assert np.array_equal(fields.cpu().numpy(), V.split_fields_host(host.numpy(), H, W, layout, bits))
    kept, made = fields[:n], fields[n:]
    for fill in (0, 1):
        V.fields_weave(kept, None if fill else made, H, W, layout, bits, V.BOTTOM, fill, out=woven)
        assert np.array_equal(woven.cpu().numpy(), V.weave_fields_host(kept.cpu().numpy(), made.cpu().numpy(), H, W, layout, bits, V.BOTTOM, fill))
    src, dst = torch.empty(n * fb, dtype=torch.uint8, device=dev).random_(), torch.empty(n * fb, dtype=torch.uint8, device=dev)
    ms = alternated_ms({"ssm_fields_split_fwd": lambda: V.fields_split(frames, H, W, layout, bits, out=fields),
                        "ssm_fields_weave_fwd": lambda: V.fields_weave(kept, made, H, W, layout, bits, V.BOTTOM, 0, out=woven),
                        "ssm_fields_weave_fwd_fill": lambda: V.fields_weave(kept, None, H, W, layout, bits, V.BOTTOM, 1, out=woven),
                        "d2d_copy_of_the_same_bytes": lambda: dst.copy_(src)}, iters, windows)
    copy = ms["d2d_copy_of_the_same_bytes"]["median"]
    touched = {"ssm_fields_split_fwd": 2 * n * fb, "ssm_fields_weave_fwd": 2 * n * fb, "ssm_fields_weave_fwd_fill": n * fb + n * fb // 2,
               "d2d_copy_of_the_same_bytes": 2 * n * fb}
    rec = {"frames": n, "frame": [H, W], "chroma": tag, "frame_bytes": fb, "ms_per_call": ms}
    for k, nbytes in touched.items():
        ideal = 1e3 * nbytes / COPY_CEILING_BYTES_PER_S
        rec[k] = {"one_touch_bytes": nbytes, "one_touch_ms": round(ideal, 4), "fraction_of_copy_ceiling": round(ideal / ms[k]["median"], 3),
                  "over_the_copy": round(ms[k]["median"] / copy, 3)}
    return rec


def bench_fps(dev, runs):
    import numpy as np
    import torch
    from ssm_amd import frames as F
    from ssm_amd import video as V
    from ssm_amd.weights import synthetic_frames_u8
    model, cfg = synthetic_model(dev)
    fh, n_fields = H // 2, 2 * CLIP_FRAMES
    base = 43          # synthetic_frames_u8 holds 43 frames at the most: the clip plays them forth and back
    rgb = synthetic_frames_u8(base, fh, W, seed=42).permute(0, 2, 3, 1).contiguous()
    matrix, crange, siting = V.default_matrix(H), V.LIMITED, V.CENTRED          # the FRAME's matrix for the 360-row fields: not synthetic_payloads
    made = torch.cat([V.frames_to_yuv(F.frames_from_u8(rgb[i:i + 8].to(dev), cfg, True), fh, W, siting, matrix, crange, cfg).cpu()
                      for i in range(0, base, 8)]).numpy()
    period = 2 * (base - 1)
    fields = made[[i % period if i % period < base else period - i % period for i in range(n_fields)]]          # 128 fields of 360 x 1280, in time order
    woven = np.concatenate([V.weave_fields_host(fields[f:f + 1], fields[f + 1:f + 2], H, W, siting, 8, V.TOP, 0) for f in range(0, n_fields, 2)])
    legs = {"deinterlace_auto_64_frames_720p_It": V.VideoInterpolator(model, cfg, n_streams=2, pairs_per_batch=1, matrix=matrix, deinterlace="auto"),
            "upsample_rate_2_128_frames_360x1280": V.VideoInterpolator(model, cfg, upsample_rate=2, n_streams=2, pairs_per_batch=1, matrix=matrix)}
    count = {}
    with tempfile.TemporaryDirectory(prefix="bench_fields_") as tmp:
        paths = {"deinterlace_auto_64_frames_720p_It": os.path.join(tmp, "interlaced.y4m"),
                 "upsample_rate_2_128_frames_360x1280": os.path.join(tmp, "progressive.y4m")}
        write_y4m(paths["deinterlace_auto_64_frames_720p_It"], woven, W, H, (25, 1), interlace="t")
        write_y4m(paths["upsample_rate_2_128_frames_360x1280"], fields, W, fh, (50, 1))

        def run(name):          # the clock starts with the files open
            with V.Y4MReader(paths[name], interlaced=True) as r, V.Y4MWriter.like(os.devnull, r, rate=V.output_rate(r.rate, 2)) as w:
                t0 = time.perf_counter()
                count[name] = legs[name].run(r, w)
                w.f.flush()
                return time.perf_counter() - t0

        secs = timed_legs(legs, run, runs, warmup=2, between=share_streams(list(legs.values())[::-1]))          # on the progressive leg's streams
    assert count == {"deinterlace_auto_64_frames_720p_It": n_fields, "upsample_rate_2_128_frames_360x1280": 2 * n_fields - 1}
    pairs = {"deinterlace_auto_64_frames_720p_It": n_fields - 2, "upsample_rate_2_128_frames_360x1280": n_fields - 1}
    per_pair = {k: statistics.median(ts) / pairs[k] for k, ts in secs.items()}
    return {"output_frames_per_s": {k: per_s(count[k], ts) for k, ts in secs.items()},
            "pairs_per_s": {k: per_s(pairs[k], ts) for k, ts in secs.items()},
            "seconds_per_run": {k: [round(t, 3) for t in ts] for k, ts in secs.items()},
            "outputs": count, "pairs": pairs,
            "deinterlace_over_progressive_time_per_pair": round(per_pair["deinterlace_auto_64_frames_720p_It"] /
                                                                per_pair["upsample_rate_2_128_frames_360x1280"], 4),
            "note": "%d fields of %dx%d (43 synthetic frames forth and back) as %d woven frames of %dx%d and as a progressive clip; file to "
                    "/dev/null, 2 streams x 1 pair, legs in turns on the same two HIP streams, %d timed runs each"
                    % (n_fields, W, fh, CLIP_FRAMES, W, H, runs)}


def run_step(step, args):
    import torch
    assert torch.cuda.is_available(), "bench_fields.py measures on the GPU; there is no CPU path"
    dev = torch.device("cuda:0")
    return bench_fps(dev, args.runs) if step == "fps" else bench_kernel(dev, step.split("_", 1)[1], args.iters, args.windows)


HEAD = ("Interlaced clips of the streamed video path (ssm_fields_split_fwd, ssm_fields_weave_fwd, VideoInterpolator(deinterlace=); DESIGN "
        "3.12).\nOne MI355X, the default precision, synthetic weights and frames.  Tool: tools/bench_fields.py (each step a process under "
        "its own time limit).\nNothing is asserted; with synthetic weights nothing can be said about quality.\n")


def main():
    args = parser("fields_bench.txt", STEPS).parse_args()
    if args.only:
        return run_only(args.only, lambda: run_step(args.only, args))
    return drive(__file__, HEAD, STEPS, args)


if __name__ == "__main__":
    sys.exit(main())
