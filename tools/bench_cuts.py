"""The scene cuts of the streamed video path (VideoInterpolator(scene_cut=)) on synthetic frames.  Driver, timer and fixture are
tools/video_bench.py's.  Two steps, each a child process under its own `timeout`, chained: the first one that fails (or runs into its
limit) ends the run.  Each step prints one JSON line:
  kernel   event-timed ssm_luma_sad_fwd (its memset included) on 7 frame pairs at 720p - frames n and n + 1 of 8 payloads in one buffer, as
           the streamed loop lays them out - beside device-to-device copies in the same run: one that reads all the bytes the kernel reads
           (and writes as many), one whose read and written bytes together are the kernel's bytes; median over `--windows` windows of
           `--iters` back-to-back calls, per call
  fps      output frames per second of wall time of VideoInterpolator.run, file to /dev/null, on a 720p clip at upsample_rate 8, in turns:
           without scene_cut and with it; 2 streams x 1 pair, both legs on the same two HIP streams (DESIGN 3.12 on why)
Nothing is asserted on the numbers.  Expectations they are there to test: the kernel sits near the copy's time for its bytes (the
accumulate kernel's 1.025 x and the tile stitch kernel's 1.16 x are the comparable figures in the project), and the stream rate with the
option lies inside the tool's own run-to-run spread (2 B per pixel read beside about 7 ms of work per pair).
Usage: python tools/bench_cuts.py [--out profiles/scene_cut_bench.txt] [--only kernel|fps] [--iters 20] [--windows 7] [--runs 3] [--frames 41]"""
import os
import sys
import tempfile
import time
from fractions import Fraction

from video_bench import call_ms, drive, parser, per_s, run_only, share_streams, synthetic_model, synthetic_payloads, timed_legs, write_y4m

STEPS = (("kernel", 180), ("fps", 600))          # step, its time limit in seconds
H, W = 720, 1280
THRESHOLD = Fraction(1, 10)          # a value for the run, not a recommendation: the synthetic clip moves steadily and holds no cut


def bench_kernel(dev, iters, windows):
    import numpy as np
    import torch
    from ssm_amd import video as V
    n = 7
    fb = V.frame_bytes(H, W, V.CENTRED)
    gen = torch.Generator(device="cpu").manual_seed(1)
    host = torch.randint(0, 256, (n + 1, fb), generator=gen, dtype=torch.uint8)
    buf = host.to(dev)
    sums = torch.empty(n, dtype=torch.int64, device=dev)
    nbytes = 2 * n * H * W          # what the kernel reads
    V.luma_sad(buf[:-1], buf[1:], H, W, out=sums)
    y = host.numpy()[:, :H * W].reshape(n + 1, H, W)
    assert sums.cpu().numpy().view(np.uint64).tolist() == V.luma_sad_host(y[:-1], y[1:]).tolist()
    src, dst = torch.empty(nbytes, dtype=torch.uint8, device=dev).random_(), torch.empty(nbytes, dtype=torch.uint8, device=dev)
    ms = call_ms(lambda: V.luma_sad(buf[:-1], buf[1:], H, W, out=sums), iters, windows)
    copy_all_ms = call_ms(lambda: dst.copy_(src), iters, windows)
    copy_half_ms = call_ms(lambda: dst[:nbytes // 2].copy_(src[:nbytes // 2]), iters, windows)
    return {"pairs": n, "plane": [H, W], "frame_bytes": fb, "bytes_read": nbytes, "ssm_luma_sad_fwd_ms": round(ms, 4),
            "d2d_copy_reading_the_same_bytes_ms": round(copy_all_ms, 4), "d2d_copy_read_plus_written_the_same_bytes_ms": round(copy_half_ms, 4),
            "sad_over_copy_reading_the_same_bytes": round(ms / copy_all_ms, 3),
            "sad_over_copy_read_plus_written_the_same_bytes": round(ms / copy_half_ms, 3), "sad_GB_per_s": round(nbytes / ms / 1e6, 1)}


def bench_fps(dev, runs, n_frames):
    from ssm_amd import video as V
    assert 2 <= n_frames <= 43, "synthetic_frames_u8 holds 43 frames of this size at the most"
    model, cfg = synthetic_model(dev)
    payloads = synthetic_payloads(n_frames, H, W, dev, cfg)
    legs = {"no_scene_cut": V.VideoInterpolator(model, cfg, upsample_rate=8, n_streams=2, pairs_per_batch=1),
            "scene_cut": V.VideoInterpolator(model, cfg, upsample_rate=8, n_streams=2, pairs_per_batch=1, scene_cut=THRESHOLD)}
    frames_written = {}
    with tempfile.TemporaryDirectory(prefix="bench_cuts_") as tmp:
        src = os.path.join(tmp, "clip.y4m")
        write_y4m(src, payloads, W, H, (30, 1))

        def run(name):          # the clock starts with the files open
            with V.Y4MReader(src) as r, V.Y4MWriter.like(os.devnull, r, rate=(240, 1)) as w:
                t0 = time.perf_counter()
                frames_written[name] = legs[name].run(r, w)
                w.f.flush()
                return time.perf_counter() - t0

        secs = timed_legs(legs, run, runs, warmup=2, between=share_streams(list(legs.values())))
    rec = {}
    for name, ts in secs.items():
        v = per_s(frames_written[name], ts)
        rec[name] = {"output_frames_per_s": v["median"], "min": v["min"], "max": v["max"], "frames_written": frames_written[name]}
    rec["scene_cut"]["cuts"] = [[i, float(s)] for i, s in legs["scene_cut"].cuts]
    rec["scene_cut_over_no_scene_cut_time_per_output_frame"] = round(rec["no_scene_cut"]["output_frames_per_s"] /
                                                                     rec["scene_cut"]["output_frames_per_s"], 4)
    rec["note"] = ("%d frames of %dx%d, upsample_rate 8, file to /dev/null, 2 streams x 1 pair, legs in turns on the same two HIP streams, %d timed "
                   "runs each; threshold %s" % (n_frames, W, H, runs, THRESHOLD))
    return rec


def run_step(step, args):
    import torch
    assert torch.cuda.is_available(), "bench_cuts.py measures on the GPU; there is no CPU path"
    dev = torch.device("cuda:0")
    return bench_kernel(dev, args.iters, args.windows) if step == "kernel" else bench_fps(dev, args.runs, args.frames)


HEAD = ("Scene cuts of the streamed video path (luma differences summed on the GPU, the decision on the writer thread; DESIGN 3.12).\n"
        "One MI355X, the default precision, synthetic weights and frames.  Tool: tools/bench_cuts.py (each step a process under its own "
        "time limit).\nExpected: the kernel near a copy's time for its bytes (accumulate kernel 1.025 x, tile stitch kernel 1.16 x); the "
        "stream rate with the option inside the run-to-run spread.  Nothing is asserted.\n")


def main():
    args = parser("scene_cut_bench.txt", STEPS, frames=41).parse_args()
    if args.only:
        return run_only(args.only, lambda: run_step(args.only, args))
    return drive(__file__, HEAD, STEPS, args)


if __name__ == "__main__":
    sys.exit(main())
