"""The shutter in linear light (VideoInterpolator(shutter_light=)) on synthetic frames; the workload is tools/bench_shutter.py's, driver,
timer and fixture are tools/video_bench.py's.  Two steps, each a child process under its own `timeout`, chained: the first one that
fails (or runs into its limit) ends the run.  Each step prints one JSON line:
  kernel   event-timed ssm_frames_accumulate_light_fwd on 8 frames at 736x1280 (init = 1, scale = 1/8: 8 planes read, one written), for
           each curve with encode = 0 and 1, beside ssm_frames_accumulate_fwd on the same frames and a device-to-device copy of the same
           bytes (read + written) in the same run: median over `--windows` windows of `--iters` back-to-back calls, per call; and the
           worst |kernel - float64 yardstick| on those frames' first 64 rows (coded values uniform in [-0.05, 1.05]) beside the bound B of
           tests/test_video_light_cpu.py
  fps      output frames per second of wall time of VideoInterpolator.run, file to /dev/null, on a 720p clip at 60:1 converted to 24:1
           (step 5/2) with shutter 180 degrees in 8 samples, in turns: shutter_light "coded" and "srgb"; 2 streams x 1 pair, both legs on
           the same two HIP streams
Nothing is asserted on the numbers.  Expectations they are there to test: the kernel stays close to the coded kernel's time (1.025 x the
copy in profiles/shutter_bench.txt), and the stream rate stays inside its run-to-run spread, since stage 2 dominates.
Usage: python tools/bench_shutter_light.py [--out profiles/shutter_light_bench.txt] [--only kernel|fps] [--iters 20] [--windows 7] [--runs 3]
       [--frames 41]"""
import ctypes
import os
import sys
import tempfile
import time

from bench_shutter import H, SAMPLES, SHUTTER, W
from video_bench import (COPY_CEILING_BYTES_PER_S, call_ms, drive, parser, per_s, run_only, share_streams, synthetic_model,
                         synthetic_payloads, timed_legs, write_y4m)

STEPS = (("kernel", 240), ("fps", 600))          # step, its time limit in seconds
CURVES = ("bt709", "srgb", "bt1886")
B = 1.2e-5          # tests/test_video_light_cpu.py


def bench_kernel(dev, iters, windows):
    import numpy as np
    import torch
    from ssm_amd import hipbind as hb
    from ssm_amd import video as V
    from ssm_amd.frames import cfg_mean_std
    n, hp, wp = 8, 736, 1280
    mean, std = cfg_mean_std(None)
    m, s = (torch.tensor(x).view(1, 3, 1, 1) for x in (mean, std))
    gen = torch.Generator(device="cpu").manual_seed(1)
    frames = (((torch.rand((n, 3, hp, wp), generator=gen) * 1.1 - 0.05) - m) / s).to(dev)          # coded values in [-0.05, 1.05]
    acc = torch.empty(1, 3, hp, wp, device=dev)
    nbytes = 4 * 3 * hp * wp * (n + 1)          # 8 planes read, one written
    src, dst = torch.randn(nbytes // 8, device=dev), torch.empty(nbytes // 8, device=dev)          # read nbytes / 2, write nbytes / 2
    copy_ms = call_ms(lambda: dst.copy_(src), iters, windows)
    coded_ms = call_ms(lambda: hb.frames_accumulate(frames, acc, 1, 0.125), iters, windows)
    rec = {"frames": n, "canvas": [hp, wp], "init": 1, "scale": 0.125, "bytes_read_and_written": nbytes,
           "d2d_copy_same_bytes_ms": round(copy_ms, 4), "ms_at_copy_ceiling": round(1e3 * nbytes / COPY_CEILING_BYTES_PER_S, 4),
           "ssm_frames_accumulate_fwd_ms": round(coded_ms, 4), "coded_over_copy": round(coded_ms / copy_ms, 3), "bound_B": B}
    rows = 64
    for name in CURVES:
        row = V.light_curve(name)
        held = [(ctypes.c_float * len(x))(*[float(y) for y in x]) for x in (mean, std, row)]          # as the streamed loop: built once
        for encode in (0, 1):
            ms = call_ms(lambda: hb.frames_accumulate_light(frames, acc, 1, 0.125, *held, encode), iters, windows)
            rec["%s_encode%d" % (name, encode)] = {"ms": round(ms, 4), "over_copy": round(ms / copy_ms, 3), "over_coded": round(ms / coded_ms, 3)}
        torch.cuda.synchronize()
        want = V.accumulate_light_host(frames[:, :, :rows].cpu().numpy(), np.zeros((1, 3, rows, wp)), 1, np.float32(0.125), mean, std, row, 1)
        rec["%s_encode1" % name]["worst_distance_from_float64"] = float("%.3g" % np.abs(acc[:, :, :rows].cpu().numpy().astype(np.float64) - want).max())
    return rec


def bench_fps(dev, runs, n_frames):
    from ssm_amd import video as V
    assert 2 <= n_frames <= 43, "synthetic_frames_u8 holds 43 frames of this size at the most"
    model, cfg = synthetic_model(dev)
    payloads = synthetic_payloads(n_frames, H, W, dev, cfg)
    legs = {light: V.VideoInterpolator(model, cfg, n_streams=2, pairs_per_batch=1, target_rate=(24, 1), shutter=SHUTTER, shutter_samples=SAMPLES,
                                       shutter_light=light) for light in ("coded", "srgb")}
    frames_written = {}
    with tempfile.TemporaryDirectory(prefix="bench_shutter_light_") as tmp:
        src = os.path.join(tmp, "clip.y4m")
        write_y4m(src, payloads, W, H, (60, 1))

        def run(name):          # the clock starts with the files open
            with V.Y4MReader(src) as r, V.Y4MWriter.like(os.devnull, r, rate=(24, 1)) as w:
                t0 = time.perf_counter()
                frames_written[name] = legs[name].run(r, w)
                w.f.flush()
                return time.perf_counter() - t0

        secs = timed_legs(legs, run, runs, warmup=2, between=share_streams(list(legs.values())))
    rec = {}
    for name, ts in secs.items():
        v = per_s(frames_written[name], ts)
        rec[name] = {"output_frames_per_s": v["median"], "min": v["min"], "max": v["max"], "frames_written": frames_written[name]}
    rec["srgb_over_coded_time_per_output_frame"] = round(rec["coded"]["output_frames_per_s"] / rec["srgb"]["output_frames_per_s"], 3)
    rec["note"] = ("%d frames of %dx%d at 60:1 -> 24:1 (step 5/2), shutter 180 degrees in %d samples, file to /dev/null, 2 streams x 1 pair, legs "
                   "in turns on the same two HIP streams, %d timed runs each" % (n_frames, W, H, SAMPLES, runs))
    return rec


def run_step(step, args):
    import torch
    assert torch.cuda.is_available(), "bench_shutter_light.py measures on the GPU; there is no CPU path"
    dev = torch.device("cuda:0")
    return bench_kernel(dev, args.iters, args.windows) if step == "kernel" else bench_fps(dev, args.runs, args.frames)


HEAD = ("Shutter in linear light of the streamed video path (sub-frames decoded to light before they are averaged on the GPU; DESIGN 3.12).\n"
        "One MI355X, the default precision, synthetic weights and frames.  Tool: tools/bench_shutter_light.py (each step a process under its "
        "own time limit).\nExpected: the kernel close to the coded kernel's time (1.025 x a copy, profiles/shutter_bench.txt); the stream rate "
        "inside its run-to-run spread, since stage 2 dominates.  Nothing is asserted.\n")


def main():
    args = parser("shutter_light_bench.txt", STEPS, frames=41).parse_args()
    if args.only:
        return run_only(args.only, lambda: run_step(args.only, args))
    return drive(__file__, HEAD, STEPS, args)


if __name__ == "__main__":
    sys.exit(main())
