"""The shutter windows (VideoInterpolator(shutter_window=)) on synthetic frames; the workload is tools/bench_shutter.py's, driver,
timers and fixture are tools/video_bench.py's.  Two steps, each a child process under its own `timeout`, chained: the first one that
fails (or runs into its limit) ends the run.  Each step prints one JSON line:
  kernel   event-timed weighted accumulate kernels on 8 frames at 736x1280 (init = 1, the triangle's weights and scale: 8 planes read, one
           written) - coded, srgb, pq and hlg (the three lights with encode = 1) - each beside its unweighted sibling on the same frames
           and a device-to-device copy of the same bytes (read + written).  The three are ALTERNATED: every one of `--windows` windows
           times `--iters` back-to-back calls of the copy, then of the sibling, then of the weighted kernel; the figures are the medians
           over the windows, per call, with the windows' min and max as the run's own spread
  fps      output frames per second of wall time of VideoInterpolator.run, file to /dev/null, on a 720p clip at 60:1 converted to 24:1
           (step 5/2) with shutter 180 degrees in 8 samples, in turns: shutter_window "box" and "triangle"; 2 streams x 1 pair, both legs
           on the same two HIP streams
Nothing is asserted on the numbers.  Expectations they are there to test: the coded weighted kernel stays at the copy's time like its
sibling (it is read-bound and the weights are scalar operands), and the stream rate stays inside its run-to-run spread, since stage 2
dominates.
Usage: python tools/bench_shutter_window.py [--out profiles/shutter_window_bench.txt] [--only kernel|fps] [--iters 20] [--windows 7]
       [--runs 3] [--frames 41]"""
import ctypes
import os
import statistics
import sys
import tempfile
import time

from bench_shutter import H, SAMPLES, SHUTTER, W
from video_bench import (COPY_CEILING_BYTES_PER_S, alternated_windows, drive, parser, per_s, run_only, share_streams, synthetic_model,
                         synthetic_payloads, timed_legs, write_y4m)

STEPS = (("kernel", 240), ("fps", 600))          # step, its time limit in seconds
WINDOW = "triangle"


def bench_kernel(dev, iters, windows):
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
    w, scale = V.shutter_window(WINDOW, n)
    wts, scale = (ctypes.c_float * n)(*[float(x) for x in w]), float(scale)          # as the binding takes them: built once
    floats = lambda x: (ctypes.c_float * len(x))(*[float(y) for y in x])
    nm = (floats(mean), floats(std))
    kind_pq, row_pq = V.hdr_light("pq")
    kind_hlg, row_hlg = V.hdr_light("hlg")
    srgb, pq, hlg = floats(V.light_curve("srgb")), floats(row_pq), floats(row_hlg)
    pairs = {"coded": (lambda: hb.frames_accumulate(frames, acc, 1, 0.125),
                       lambda: hb.frames_accumulate(frames, acc, 1, scale, weights=wts)),
             "srgb": (lambda: hb.frames_accumulate_light(frames, acc, 1, 0.125, *nm, srgb, 1),
                      lambda: hb.frames_accumulate_light(frames, acc, 1, scale, *nm, srgb, 1, weights=wts)),
             "pq": (lambda: hb.frames_accumulate_hdr(frames, acc, 1, 0.125, *nm, kind_pq, pq, 1),
                    lambda: hb.frames_accumulate_hdr(frames, acc, 1, scale, *nm, kind_pq, pq, 1, weights=wts)),
             "hlg": (lambda: hb.frames_accumulate_hdr(frames, acc, 1, 0.125, *nm, kind_hlg, hlg, 1),
                     lambda: hb.frames_accumulate_hdr(frames, acc, 1, scale, *nm, kind_hlg, hlg, 1, weights=wts))}
    rec = {"frames": n, "canvas": [hp, wp], "init": 1, "window": WINDOW, "weights": [float(x) for x in w], "scale": scale,
           "bytes_read_and_written": nbytes, "ms_at_copy_ceiling": round(1e3 * nbytes / COPY_CEILING_BYTES_PER_S, 4),
           "iters_per_window": iters, "windows": windows}
    for name, (plain, weighted) in pairs.items():
        t = alternated_windows({"copy": lambda: dst.copy_(src), "unweighted": plain, "weighted": weighted}, iters, windows)
        t = {k: (statistics.median(v), min(v), max(v)) for k, v in t.items()}          # unrounded: the ratios below are of these
        rec[name] = {k: {"ms": round(v[0], 4), "min": round(v[1], 4), "max": round(v[2], 4)} for k, v in t.items()}
        rec[name]["weighted_over_unweighted"] = round(t["weighted"][0] / t["unweighted"][0], 3)
        rec[name]["weighted_over_copy"] = round(t["weighted"][0] / t["copy"][0], 3)
        rec[name]["unweighted_over_copy"] = round(t["unweighted"][0] / t["copy"][0], 3)
    return rec


def bench_fps(dev, runs, n_frames):
    from ssm_amd import video as V
    assert 2 <= n_frames <= 43, "synthetic_frames_u8 holds 43 frames of this size at the most"
    model, cfg = synthetic_model(dev)
    payloads = synthetic_payloads(n_frames, H, W, dev, cfg)
    legs = {window: V.VideoInterpolator(model, cfg, n_streams=2, pairs_per_batch=1, target_rate=(24, 1), shutter=SHUTTER, shutter_samples=SAMPLES,
                                        shutter_window=window) for window in ("box", WINDOW)}
    frames_written = {}
    with tempfile.TemporaryDirectory(prefix="bench_shutter_window_") as tmp:
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
    rec["%s_over_box_time_per_output_frame" % WINDOW] = round(rec["box"]["output_frames_per_s"] / rec[WINDOW]["output_frames_per_s"], 3)
    rec["note"] = ("%d frames of %dx%d at 60:1 -> 24:1 (step 5/2), shutter 180 degrees in %d samples, file to /dev/null, 2 streams x 1 pair, legs "
                   "in turns on the same two HIP streams, %d timed runs each" % (n_frames, W, H, SAMPLES, runs))
    return rec


def run_step(step, args):
    import torch
    assert torch.cuda.is_available(), "bench_shutter_window.py measures on the GPU; there is no CPU path"
    dev = torch.device("cuda:0")
    return bench_kernel(dev, args.iters, args.windows) if step == "kernel" else bench_fps(dev, args.runs, args.frames)


HEAD = ("Shutter windows of the streamed video path (weighted sums of the sub-frames on the GPU; DESIGN 3.12).\n"
        "One MI355X, the default precision, synthetic weights and frames.  Tool: tools/bench_shutter_window.py (each step a process under its "
        "own time limit;\nthe copy, the unweighted kernel and the weighted kernel alternate window by window in one run).\nExpected: the coded "
        "weighted kernel at the copy's time, like its sibling; the stream rate inside its run-to-run spread, since stage 2 dominates.\n"
        "Nothing is asserted.\n")


def main():
    args = parser("shutter_window_bench.txt", STEPS, frames=41).parse_args()
    if args.only:
        return run_only(args.only, lambda: run_step(args.only, args))
    return drive(__file__, HEAD, STEPS, args)


if __name__ == "__main__":
    sys.exit(main())
