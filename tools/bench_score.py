"""Hold-out scoring of the streamed video path (ssm_amd/video_score.py) on synthetic frames.  Driver, timer and fixture
are tools/video_bench.py's.  Three steps, each a child process under its own `timeout`, chained: the first one that fails (or runs into
its limit) ends the run.  Each step prints one JSON line:
  kernel_420jpeg, kernel_422p10
           event-timed ssm_plane_sse_fwd (its memset included) on 7 frame pairs at 720p - frames n and n + 1 of 8 payloads in one buffer -
           beside device-to-device copies in the same run: one of N frame_bytes, which reads and writes together the 2 N frame_bytes the
           kernel reads (the same bytes moved, each touched once), and one of 2 N frame_bytes, which reads all the bytes the kernel reads
           and writes as many; and the call's one-touch bytes as a fraction of the 6.29 TB/s copy ceiling (tools/bench_video.py).  Median
           over `--windows` windows of `--iters` back-to-back calls, per call.  The sums are checked against the yardstick first.
  fps      frames per second of wall time on a 65-frame 720p clip (the 43 synthetic frames played forth and back), file to /dev/null, in
           turns on the same two HIP streams: HoldOutScorer(hold=8) over the 65 frames - INPUT frames read per second, and the 65 output
           frames of the decimated clip per second - beside VideoInterpolator(upsample_rate=8) on the 9 kept frames, output frames per
           second; 2 streams x 1 pair.  The scorer reads 8 times the frames and uploads them; what it runs on the GPU beside the tool's
           own passes is 2 + 1 small calls per pass.
Nothing is asserted on the numbers; no one had measured either.  With synthetic weights the PSNR values say nothing about quality.
Usage: python tools/bench_score.py [--out profiles/video_score_bench.txt] [--only STEP] [--iters 20] [--windows 7] [--runs 3]"""
import os
import statistics
import sys
import tempfile
import time

from video_bench import (COPY_CEILING_BYTES_PER_S, call_ms, drive, parser, per_s, run_only, share_streams, synthetic_model,
                         synthetic_payloads, timed_legs, write_y4m)

STEPS = (("kernel_420jpeg", 180), ("kernel_422p10", 180), ("fps", 600))          # step, its time limit in seconds
H, W, HOLD, CLIP_FRAMES = 720, 1280, 8, 65


def bench_kernel(dev, tag, iters, windows):
    import numpy as np
    import torch
    from ssm_amd import video as V
    from ssm_amd import video_score as S
    n = 7
    layout, bits = V.EXTENDED_TAGS[tag]
    fb = V.frame_bytes(H, W, layout, bits)
    gen = torch.Generator(device="cpu").manual_seed(1)
    host = torch.randint(0, 256, (n + 1, fb), generator=gen, dtype=torch.uint8)
    buf = host.to(dev)
    sums = torch.empty(n, 3, dtype=torch.int64, device=dev)
    nbytes = 2 * n * fb          # what the kernel reads
    S.plane_sse(buf[:-1], buf[1:], H, W, layout, bits, out=sums)
    assert sums.cpu().numpy().view(np.uint64).tolist() == S.plane_sse_host(host.numpy()[:-1], host.numpy()[1:], H, W, layout, bits).tolist()
    src, dst = torch.empty(nbytes, dtype=torch.uint8, device=dev).random_(), torch.empty(nbytes, dtype=torch.uint8, device=dev)
    ms = call_ms(lambda: S.plane_sse(buf[:-1], buf[1:], H, W, layout, bits, out=sums), iters, windows)
    copy_all_ms = call_ms(lambda: dst.copy_(src), iters, windows)
    copy_half_ms = call_ms(lambda: dst[:nbytes // 2].copy_(src[:nbytes // 2]), iters, windows)
    ideal_ms = 1e3 * nbytes / COPY_CEILING_BYTES_PER_S
    return {"pairs": n, "frame": [H, W], "chroma": tag, "frame_bytes": fb, "bytes_read": nbytes, "ssm_plane_sse_fwd_ms": round(ms, 4),
            "d2d_copy_of_N_frame_bytes_moving_the_same_bytes_ms": round(copy_half_ms, 4),
            "d2d_copy_of_2N_frame_bytes_reading_the_same_bytes_ms": round(copy_all_ms, 4),
            "sse_over_copy_moving_the_same_bytes": round(ms / copy_half_ms, 3),
            "sse_over_copy_reading_the_same_bytes": round(ms / copy_all_ms, 3),
            "sse_GB_per_s": round(nbytes / ms / 1e6, 1), "one_touch_bytes": nbytes, "one_touch_ms": round(ideal_ms, 4),
            "fraction_of_copy_ceiling": round(ideal_ms / ms, 3)}


def bench_fps(dev, runs):
    from ssm_amd import video as V
    from ssm_amd import video_score as S
    model, cfg = synthetic_model(dev)
    base = 43          # synthetic_frames_u8 holds 43 frames of this size at the most: the clip plays them forth and back
    made = synthetic_payloads(base, H, W, dev, cfg)
    order = [i if i < base else 2 * (base - 1) - i for i in range(CLIP_FRAMES)]
    payloads = made[order]
    scorer = S.HoldOutScorer(model, cfg, HOLD, n_streams=2, pairs_per_batch=1)
    tool = V.VideoInterpolator(model, cfg, upsample_rate=HOLD, n_streams=2, pairs_per_batch=1)
    last = {}
    with tempfile.TemporaryDirectory(prefix="bench_score_") as tmp:
        full, kept = os.path.join(tmp, "clip.y4m"), os.path.join(tmp, "kept.y4m")
        write_y4m(full, payloads, W, H, (240, 1))
        write_y4m(kept, payloads[::HOLD], W, H, (30, 1))
        legs = {"hold_out_scorer": (scorer, full, {}), "video_interpolator": (tool, kept, {"rate": (240, 1)})}

        def run(name):          # the clock starts with the files open
            runner, path, kw = legs[name]
            with V.Y4MReader(path) as r, V.Y4MWriter.like(os.devnull, r, **kw) as w:
                t0 = time.perf_counter()
                last[name] = runner.run(r, w)
                w.f.flush()
                return time.perf_counter() - t0

        secs = timed_legs(legs, run, runs, warmup=2, between=share_streams([tool, scorer.vi]))          # on the tool's streams
    res = last["hold_out_scorer"]
    assert res.written == last["video_interpolator"] == CLIP_FRAMES and res.scored == (CLIP_FRAMES - 1) // HOLD * (HOLD - 1)
    rec = {"hold_out_scorer": {"input_frames_read_per_s": per_s(res.frames_read, secs["hold_out_scorer"]),
                               "output_frames_per_s": per_s(res.written, secs["hold_out_scorer"]),
                               "frames_read": res.frames_read, "scored": res.scored, "trailing": res.trailing},
           "video_interpolator_on_the_decimated_clip": {"output_frames_per_s": per_s(last["video_interpolator"], secs["video_interpolator"]),
                                                        "frames_written": last["video_interpolator"]},
           "scorer_over_tool_time_per_output_frame": round(statistics.median(secs["hold_out_scorer"]) / statistics.median(secs["video_interpolator"]), 4),
           "pooled_psnr_db_synthetic_weights_no_statement_on_quality": {k: {p: round(v, 3) for p, v in d.items()}
                                                                        for k, d in res.pooled().items() if k != "frames"},
           "note": "%d frames of %dx%d (43 synthetic frames forth and back), hold %d, file to /dev/null, 2 streams x 1 pair, legs in turns on the "
                   "same two HIP streams, %d timed runs each" % (CLIP_FRAMES, W, H, HOLD, runs)}
    return rec


def run_step(step, args):
    import torch
    assert torch.cuda.is_available(), "bench_score.py measures on the GPU; there is no CPU path"
    dev = torch.device("cuda:0")
    return bench_fps(dev, args.runs) if step == "fps" else bench_kernel(dev, step.split("_", 1)[1], args.iters, args.windows)


HEAD = ("Hold-out scoring of the streamed video path (squared differences summed per plane on the GPU, rows made on the writer thread; "
        "DESIGN 3.12).\nOne MI355X, the default precision, synthetic weights and frames.  Tool: tools/bench_score.py (each step a process "
        "under its own time limit).\nNothing is asserted; the PSNR values of synthetic weights say nothing about quality.\n")


def main():
    args = parser("video_score_bench.txt", STEPS).parse_args()
    if args.only:
        return run_only(args.only, lambda: run_step(args.only, args))
    return drive(__file__, HEAD, STEPS, args)


if __name__ == "__main__":
    sys.exit(main())
