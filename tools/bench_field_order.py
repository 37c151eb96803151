"""The field probe of the streamed video path (ssm_amd/video.py) on synthetic frames.  Driver, timers and model are
tools/video_bench.py's: three steps, each a child process under its own `timeout`, chained - the first one that fails (or runs into its
limit) ends the run.  Each step prints one JSON line:
  kernel_bytes, kernel_words
           event-timed ssm_field_order_sums_fwd on 7 frames (rows n - 1, n, n + 1 of 9 payloads of 720 x 1280, 4:2:0, 8-bit or 10-bit in
           words), beside ssm_field_diff_fwd on the same planes (rows n + 1 against rows n) and a device-to-device copy of as many bytes as
           the new call reads (3 luma planes per frame), ALTERNATED in one run: a round times every call once, window after window.  Per
           call: the median over `--windows` rounds of `--iters` back-to-back calls, with the least and the largest; the bytes the call
           reads as a fraction of the 6.29 TB/s copy ceiling (tools/bench_video.py).  The sums are checked against the yardsticks first.
  fps      output frames per second of wall time, file to /dev/null, in turns: a 64-frame 720 x 1280 top-field-first clip under an Ip
           header through VideoInterpolator(deinterlace="auto", field_probe=True) beside deinterlace="tff" on the same file (the same 128
           outputs): what the probe costs the stream.  A run of the first leg makes its FieldOrderSource, pinned buffers included.
Nothing is asserted on the numbers.  With synthetic weights nothing can be said about quality.  Nothing was traced: no kernel trace, no
counters; the times are device events (kernels) and the host's clock around whole runs (stream).
Usage: python tools/bench_field_order.py [--out profiles/field_order_bench.txt] [--only STEP] [--iters 20] [--windows 7] [--runs 3]"""
import os
import statistics
import sys
import tempfile
import time

from video_bench import COPY_CEILING_BYTES_PER_S, alternated_ms, drive, parser, per_s, run_only, synthetic_model, timed_legs, write_y4m

STEPS = (("kernel_bytes", 180), ("kernel_words", 180), ("fps", 600))          # step, its time limit in seconds
H, W, CLIP_FRAMES = 720, 1280, 64
TAGS = {"kernel_bytes": "420jpeg", "kernel_words": "420p10"}


def bench_kernel(dev, tag, iters, windows):
    import numpy as np
    import torch
    from ssm_amd import video as V
    n = 7
    layout, bits = V.EXTENDED_TAGS[tag]
    fb, luma = V.frame_bytes(H, W, layout, bits), H * W * V.sample_bytes(bits)
    gen = torch.Generator(device="cpu").manual_seed(1)
    host = torch.randint(0, 256, (n + 2, fb), generator=gen, dtype=torch.uint8)
    frames = host.to(dev)
    prev, cur, nxt = frames[:-2], frames[1:-1], frames[2:]
    sums = torch.empty(n, 3, dtype=torch.int64, device=dev)
    V.field_order_sums(prev, cur, nxt, H, W, bits, out=sums)
    hn = host.numpy()
    assert np.array_equal(sums.cpu().numpy().view(np.uint64), V.field_order_sums_host(hn[:-2], hn[1:-1], hn[2:], H, W, bits))
    diff = torch.empty(n, 2, dtype=torch.int64, device=dev)
    V.field_diff(nxt, cur, H, W, bits, out=diff)
    assert np.array_equal(diff.cpu().numpy().view(np.uint64), V.field_diff_host(hn[2:], hn[1:-1], H, W, bits))
    src, dst = torch.empty(3 * n * luma, dtype=torch.uint8, device=dev).random_(), torch.empty(3 * n * luma, dtype=torch.uint8, device=dev)
    calls = {"ssm_field_order_sums_fwd": lambda: V.field_order_sums(prev, cur, nxt, H, W, bits, out=sums),
             "ssm_field_diff_fwd": lambda: V.field_diff(nxt, cur, H, W, bits, out=diff),
             "d2d_copy_of_as_many_bytes": lambda: dst.copy_(src)}
    ms = alternated_ms(calls, iters, windows)
    copy = ms["d2d_copy_of_as_many_bytes"]["median"]
    read = {"ssm_field_order_sums_fwd": 3 * n * luma, "ssm_field_diff_fwd": 2 * n * luma, "d2d_copy_of_as_many_bytes": 3 * n * luma}
    rec = {"frames": n, "frame": [H, W], "chroma": tag, "frame_bytes": fb, "bytes_of_the_operands": read, "ms_per_call": ms}
    for k in calls:
        ideal = 1e3 * read[k] / COPY_CEILING_BYTES_PER_S
        rec[k] = {"operand_bytes_at_the_copy_ceiling_ms": round(ideal, 4), "fraction_of_copy_ceiling": round(ideal / ms[k]["median"], 3),
                  "over_the_copy": round(ms[k]["median"] / copy, 3)}
    rec["field_order_sums_over_field_diff"] = round(ms["ssm_field_order_sums_fwd"]["median"] / ms["ssm_field_diff_fwd"]["median"], 3)
    return rec


def bench_fps(dev, runs):
    import numpy as np
    from ssm_amd import video as V
    model, cfg = synthetic_model(dev)
    matrix, siting = V.default_matrix(H), V.CENTRED
    # the moving texture of the field-order tests (tests/field_clips.py), top field first: frame i's even rows at field time 2i, its odd
    # rows at 2i + 1; chroma at mid-grey
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    clip = np.full((CLIP_FRAMES, V.frame_bytes(H, W, siting)), 128, np.uint8)
    luma = V.split_planes(clip, H, W, siting)[0]
    for i in range(CLIP_FRAMES):
        for parity in (0, 1):
            t = 2 * i + parity
            v = 128 + 60 * np.sin((x - 3 * t) / 5 + 0.3 * np.sin(y / 7)) + 40 * np.sin((y - 1.5 * t) / 9)
            luma[i, parity::2] = np.clip(np.rint(v), 0, 255).astype(np.uint8)[parity::2]
    rate = (30000, 1001)
    legs = {"deinterlace_auto_field_probe_64_frames_720p": dict(deinterlace="auto", field_probe=True),
            "deinterlace_tff_64_frames_720p": dict(deinterlace="tff")}
    vis = {k: V.VideoInterpolator(model, cfg, n_streams=2, pairs_per_batch=1, matrix=matrix, **kw) for k, kw in legs.items()}
    count = {}
    with tempfile.TemporaryDirectory(prefix="bench_field_order_") as tmp:
        path = os.path.join(tmp, "ip.y4m")
        write_y4m(path, clip, W, H, rate, interlace="p")

        def run(name):          # the clock runs while the files are opened and closed
            t0 = time.perf_counter()
            with V.Y4MReader(path, interlaced=True) as r:
                with V.Y4MWriter.like(os.devnull, r, rate=V.output_rate(r.rate, 2)) as w:
                    count[name] = vis[name].run(r, w)
                    w.f.flush()
            return time.perf_counter() - t0

        secs = timed_legs(legs, run, runs)
    probe = vis["deinterlace_auto_field_probe_64_frames_720p"].field_probe
    assert count == {k: 2 * CLIP_FRAMES for k in legs} and (probe.verdict, probe.order) == ("tff", "tff"), (count, probe)
    a, b = legs
    return {"output_frames_per_s": {k: per_s(count[k], ts) for k, ts in secs.items()},
            "seconds_per_run": {k: [round(t, 3) for t in ts] for k, ts in secs.items()},
            "outputs": count, "field_probe": {"verdict": probe.verdict, "counts": list(probe.counts), "note": probe.note},
            "probed_over_named_time_per_run": round(statistics.median(secs[a]) / statistics.median(secs[b]), 4),
            "note": "%d frames of %dx%d of a moving texture woven top field first, under an Ip header; file to /dev/null, "
                    "2 streams x 1 pair, legs in turns, %d timed runs each; a run opens its file and, the first leg, makes its "
                    "FieldOrderSource and probes 48 frames" % (CLIP_FRAMES, W, H, runs)}


def run_step(step, args):
    import torch
    assert torch.cuda.is_available(), "bench_field_order.py measures on the GPU; there is no CPU path"
    dev = torch.device("cuda:0")
    return bench_fps(dev, args.runs) if step == "fps" else bench_kernel(dev, TAGS[step], args.iters, args.windows)


HEAD = ("The field probe of the streamed video path (ssm_field_order_sums_fwd, FieldOrderSource, --field_probe; DESIGN 3.12).\nOne MI355X, "
        "the default precision, synthetic weights and frames.  Tool: tools/bench_field_order.py (each step a process under its own time "
        "limit).\nNothing is asserted; nothing was traced (no kernel trace, no counters); with synthetic weights nothing can be said about "
        "quality.\n")


def main():
    args = parser("field_order_bench.txt", STEPS).parse_args()
    if args.only:
        return run_only(args.only, lambda: run_step(args.only, args))
    return drive(__file__, HEAD, STEPS, args)


if __name__ == "__main__":
    sys.exit(main())
