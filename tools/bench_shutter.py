"""The shutter of the streamed video path (VideoInterpolator(shutter=, shutter_samples=)) on synthetic frames.  Driver, timer and
fixture are tools/video_bench.py's.  Two steps, each a child process under its own `timeout`, chained: the first one that fails (or runs
into its limit) ends the run.  Each step prints one JSON line:
  kernel   event-timed ssm_frames_accumulate_fwd on 8 frames at 736x1280 (init = 1, scale = 1/8: 8 planes read, one written) beside a
           device-to-device copy of the same bytes (read + written) in the same run: median over `--windows` windows of `--iters`
           back-to-back calls, per call, and the fractions of the 6.29 TB/s copy ceiling
  fps      output frames per second of wall time of VideoInterpolator.run, file to /dev/null, on a 720p clip at 60:1 converted to 24:1
           (step 5/2), in turns: without a shutter, and with shutter 180 degrees in 8 samples; 2 streams x 1 pair, both legs on the same two
           HIP streams (DESIGN 3.12 on why), with the stage-2 entries each leg runs per output frame
Nothing is asserted on the numbers.  Expectations they are there to test: the kernel sits near the copy's time for its bytes (the tile
stitch kernel's 1.16 x is the one comparable figure in the project), and the run with a shutter costs in proportion to the stage-2 entries
it adds.
Usage: python tools/bench_shutter.py [--out profiles/shutter_bench.txt] [--only kernel|fps] [--iters 20] [--windows 7] [--runs 3] [--frames 41]"""
import os
import sys
import tempfile
import time
from fractions import Fraction

from video_bench import (COPY_CEILING_BYTES_PER_S, call_ms, drive, parser, per_s, run_only, share_streams, synthetic_model,
                         synthetic_payloads, timed_legs, write_y4m)

STEPS = (("kernel", 180), ("fps", 600))          # step, its time limit in seconds
H, W = 720, 1280
SHUTTER, SAMPLES = Fraction(1, 2), 8


def bench_kernel(dev, iters, windows):
    import torch
    from ssm_amd import hipbind as hb
    n, hp, wp = 8, 736, 1280
    gen = torch.Generator(device="cpu").manual_seed(1)
    frames = torch.randn((n, 3, hp, wp), generator=gen).to(dev)
    acc = torch.empty(1, 3, hp, wp, device=dev)
    nbytes = 4 * 3 * hp * wp * (n + 1)          # 8 planes read, one written
    src, dst = torch.randn(nbytes // 8, device=dev), torch.empty(nbytes // 8, device=dev)          # read nbytes / 2, write nbytes / 2
    ms = call_ms(lambda: hb.frames_accumulate(frames, acc, 1, 0.125), iters, windows)
    copy_ms = call_ms(lambda: dst.copy_(src), iters, windows)
    ideal = 1e3 * nbytes / COPY_CEILING_BYTES_PER_S
    return {"frames": n, "canvas": [hp, wp], "init": 1, "scale": 0.125, "bytes_read_and_written": nbytes,
            "ssm_frames_accumulate_fwd_ms": round(ms, 4), "d2d_copy_same_bytes_ms": round(copy_ms, 4), "ms_at_copy_ceiling": round(ideal, 4),
            "accumulate_fraction_of_copy_ceiling": round(ideal / ms, 3), "copy_fraction_of_copy_ceiling": round(ideal / copy_ms, 3),
            "accumulate_over_copy": round(ms / copy_ms, 3)}


def bench_fps(dev, runs, n_frames):
    from ssm_amd import video as V
    assert 2 <= n_frames <= 43, "synthetic_frames_u8 holds 43 frames of this size at the most"
    model, cfg = synthetic_model(dev)
    payloads = synthetic_payloads(n_frames, H, W, dev, cfg)
    legs = {"no_shutter": V.VideoInterpolator(model, cfg, n_streams=2, pairs_per_batch=1, target_rate=(24, 1)),
            "shutter_180_in_8": V.VideoInterpolator(model, cfg, n_streams=2, pairs_per_batch=1, target_rate=(24, 1), shutter=SHUTTER,
                                                    shutter_samples=SAMPLES)}
    tls = {name: vi.timeline((60, 1)) for name, vi in legs.items()}
    pairs_run = {name: sum(1 for i in range(n_frames - 1) if tl.count(i)) for name, tl in tls.items()}
    frames_written = {}
    with tempfile.TemporaryDirectory(prefix="bench_shutter_") as tmp:
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
        rec[name] = {"output_frames_per_s": v["median"], "min": v["min"], "max": v["max"], "frames_written": frames_written[name],
                     "pairs_run": pairs_run[name], "slots": tls[name].slots, "stage2_entries": pairs_run[name] * tls[name].slots}
    a, b = rec["no_shutter"], rec["shutter_180_in_8"]
    rec["shutter_over_no_shutter_time_per_output_frame"] = round(a["output_frames_per_s"] / b["output_frames_per_s"], 3)
    rec["shutter_over_no_shutter_stage2_entries"] = round(b["stage2_entries"] / max(a["stage2_entries"], 1), 3)
    rec["note"] = ("%d frames of %dx%d at 60:1 -> 24:1 (step 5/2), file to /dev/null, 2 streams x 1 pair, legs in turns on the same two HIP streams, "
                   "%d timed runs each; stage-2 entries = pairs that run x slots (stage 1 runs once per pair that runs)" % (n_frames, W, H, runs))
    return rec


def run_step(step, args):
    import torch
    assert torch.cuda.is_available(), "bench_shutter.py measures on the GPU; there is no CPU path"
    dev = torch.device("cuda:0")
    return bench_kernel(dev, args.iters, args.windows) if step == "kernel" else bench_fps(dev, args.runs, args.frames)


HEAD = ("Shutter of the streamed video path (shutter = open fraction of the output interval, samples averaged on the GPU; DESIGN 3.12).\n"
        "One MI355X, the default precision, synthetic weights and frames.  Tool: tools/bench_shutter.py (each step a process under its own "
        "time limit).\nExpected: the kernel near the copy's time for its bytes (the tile stitch kernel: 1.16 x); the run with a shutter "
        "costs in proportion to the stage-2 entries it adds.  Nothing is asserted.\n")


def main():
    args = parser("shutter_bench.txt", STEPS, frames=41).parse_args()
    if args.only:
        return run_only(args.only, lambda: run_step(args.only, args))
    return drive(__file__, HEAD, STEPS, args)


if __name__ == "__main__":
    sys.exit(main())
