"""The shutter in the light of HDR clips (VideoInterpolator(shutter_light="pq"|"hlg")) on synthetic frames.  Driver and timer are
tools/video_bench.py's.  One step, a child process under its own `timeout`; a failure (or the limit) ends the run.  It prints one
JSON line:
  kernel   event-timed ssm_frames_accumulate_hdr_fwd on 8 frames at 736x1280 (init = 1, scale = 1/8: 8 planes read, one written), for pq
           and hlg with encode = 0 and 1, and three reference calls alternated with them in the same run: ssm_frames_accumulate_light_fwd
           (srgb, encode = 0 and 1), ssm_frames_accumulate_fwd on the same frames, and a device-to-device copy of the same bytes (read +
           written).  `--rounds` rounds; in each, every call is timed once (median over `--windows` windows of `--iters` back-to-back calls,
           per call), in the same order; a call's figure is the median of its rounds, with their minimum and maximum - the runs' own
           spread, which is what a ratio to the srgb kernel is to be read against.  And the worst |kernel - float64 yardstick| on those
           frames' first 64 rows (coded values uniform in [-0.05, 1.05]) beside the bounds B of tests/test_video_hdr_cpu.py
Nothing is asserted on the numbers.  The expectation they are there to test: the call stays bandwidth-bound, close to the srgb kernel's
time, although PQ has four powers where sRGB has two.
Usage: python tools/bench_shutter_hdr.py [--out profiles/shutter_hdr_bench.txt] [--only kernel] [--iters 20] [--windows 5] [--rounds 3]"""
import ctypes
import statistics
import sys

from video_bench import COPY_CEILING_BYTES_PER_S, call_ms, drive, parser, run_only

STEPS = (("kernel", 300),)          # step, its time limit in seconds
NAMES = ("pq", "hlg")
B = {"pq": 2.2e-4, "hlg": 3.4e-6}          # tests/test_video_hdr_cpu.py


def bench_kernel(dev, iters, windows, rounds):
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
    c_arr = lambda x: (ctypes.c_float * len(x))(*[float(y) for y in x])          # as the streamed loop: built once
    cm, cs, srgb = c_arr(mean), c_arr(std), c_arr(V.light_curve("srgb"))
    calls = {"d2d_copy_same_bytes": lambda: dst.copy_(src),
             "ssm_frames_accumulate_fwd": lambda: hb.frames_accumulate(frames, acc, 1, 0.125)}
    for encode in (0, 1):
        calls["srgb_encode%d" % encode] = lambda e=encode: hb.frames_accumulate_light(frames, acc, 1, 0.125, cm, cs, srgb, e)
        for name in NAMES:
            kind, row = V.hdr_light(name)
            calls["%s_encode%d" % (name, encode)] = lambda e=encode, k=kind, r=c_arr(row): hb.frames_accumulate_hdr(frames, acc, 1, 0.125, cm, cs, k, r, e)
    seen = {k: [] for k in calls}
    for _ in range(rounds):          # alternated: every call once per round
        for k, fn in calls.items():
            seen[k].append(call_ms(fn, iters, windows))
    med = {k: statistics.median(v) for k, v in seen.items()}
    rec = {"frames": n, "canvas": [hp, wp], "init": 1, "scale": 0.125, "bytes_read_and_written": nbytes, "rounds": rounds,
           "ms_at_copy_ceiling": round(1e3 * nbytes / COPY_CEILING_BYTES_PER_S, 4), "bounds_B": B}
    for k, v in seen.items():
        rec[k] = {"ms": round(med[k], 4), "min": round(min(v), 4), "max": round(max(v), 4), "over_copy": round(med[k] / med["d2d_copy_same_bytes"], 3)}
        if k[:-1].endswith("_encode") and not k.startswith("srgb"):
            rec[k]["over_srgb"] = round(med[k] / med["srgb_encode" + k[-1]], 3)
    lo, hi = min(seen["srgb_encode1"]), max(seen["srgb_encode1"])
    rec["srgb_encode1_spread"] = round(hi / lo, 3)
    rows = 64
    for name in NAMES:
        kind, row = V.hdr_light(name)
        hb.frames_accumulate_hdr(frames, acc, 1, 0.125, mean, std, kind, row, 1)
        torch.cuda.synchronize()
        want = V.accumulate_hdr_host(frames[:, :, :rows].cpu().numpy(), np.zeros((1, 3, rows, wp)), 1, np.float32(0.125), mean, std, name, 1)
        rec["%s_encode1" % name]["worst_distance_from_float64"] = float("%.3g" % np.abs(acc[:, :, :rows].cpu().numpy().astype(np.float64) - want).max())
    return rec


def run_step(step, args):
    import torch
    assert torch.cuda.is_available(), "bench_shutter_hdr.py measures on the GPU; there is no CPU path"
    return bench_kernel(torch.device("cuda:0"), args.iters, args.windows, args.rounds)


HEAD = ("Shutter in the light of HDR clips in the streamed video path (sub-frames decoded by the BT.2100 PQ EOTF or the inverse HLG OETF before "
        "they are averaged on the GPU; DESIGN 3.12).\nOne MI355X, synthetic frames.  Tool: tools/bench_shutter_hdr.py (the step is a process "
        "under its own time limit).\nExpected: the call close to the srgb light kernel's time in the same run, bandwidth-bound.  Nothing is "
        "asserted.\n")


def main():
    args = parser("shutter_hdr_bench.txt", STEPS, windows=5, runs=None, rounds=3).parse_args()          # whole runs are not timed: no --runs
    if args.only:
        return run_only(args.only, lambda: run_step(args.only, args))
    return drive(__file__, HEAD, STEPS, args)


if __name__ == "__main__":
    sys.exit(main())
