"""Repair of repeated frames of the streamed video path (ssm_amd/video.py) on synthetic frames.  Driver, timers and fixture are
tools/video_bench.py's: three steps, each a child process under its own `timeout`, chained - the first one that fails (or runs into
its limit) ends the run.  Each step prints one JSON line:
  kernel_bytes, kernel_words
           event-timed ssm_block_sad_fwd on 7 frame pairs (rows n + 1 against rows n of 8 payloads of 720 x 1280, 420jpeg or 422p10),
           beside ssm_plane_sse_fwd on the same operands and a device-to-device copy of as many bytes as the calls read, ALTERNATED in
           one run: a round times every call once, window after window.  Per call: the median over `--windows` rounds of `--iters`
           back-to-back calls, with the least and the largest; the bytes the call reads as a fraction of the 6.29 TB/s copy ceiling
           (tools/bench_video.py).  The words are checked against the yardstick first.
  fps      output frames per second of wall time, file to /dev/null, in turns on one box: a 720 x 1280 clip made by repeating the frames
           of a 26-frame base clip 2, 3, 2, 3, ... times (65 frames) through VideoInterpolator(dedup=True, upsample_rate=1) - 25 repaired
           pairs, 37 synthesised frames - beside the base clip through upsample_rate=2 (25 pairs, 25 synthesised frames): what the
           repair costs per synthesised frame, the repeat test included.  A run of the first leg makes its RepeatSource, pinned buffers
           included.
Nothing is asserted on the numbers.  With synthetic weights nothing can be said about quality.
Usage: python tools/bench_dedup.py [--out profiles/dedup_bench.txt] [--only STEP] [--iters 20] [--windows 7] [--runs 3]"""
import os
import statistics
import sys
import tempfile
import time

from video_bench import (COPY_CEILING_BYTES_PER_S, alternated_ms, drive, parser, per_s, run_only, synthetic_model, synthetic_payloads,
                         timed_legs, write_y4m)

STEPS = (("kernel_bytes", 180), ("kernel_words", 180), ("fps", 600))          # step, its time limit in seconds
H, W, BASE_FRAMES = 720, 1280, 26
TAGS = {"kernel_bytes": "420jpeg", "kernel_words": "422p10"}


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
    frames = host.to(dev)
    new, old = frames[1:], frames[:-1]
    words = torch.empty(n, 3, 2, dtype=torch.int64, device=dev)
    V.block_sad(new, old, H, W, layout, bits, out=words)
    assert np.array_equal(words.cpu().numpy().view(np.uint64), V.block_sad_host(host.numpy()[1:], host.numpy()[:-1], H, W, layout, bits))
    sse = torch.empty(n, 3, dtype=torch.int64, device=dev)
    src, dst = torch.empty(n * fb, dtype=torch.uint8, device=dev).random_(), torch.empty(n * fb, dtype=torch.uint8, device=dev)
    calls = {"ssm_block_sad_fwd": lambda: V.block_sad(new, old, H, W, layout, bits, out=words),
             "ssm_plane_sse_fwd": lambda: S.plane_sse(new, old, H, W, layout, bits, out=sse),
             "d2d_copy_of_as_many_bytes": lambda: dst.copy_(src)}
    ms = alternated_ms(calls, iters, windows)
    copy = ms["d2d_copy_of_as_many_bytes"]["median"]
    ideal = 1e3 * 2 * n * fb / COPY_CEILING_BYTES_PER_S
    rec = {"pairs": n, "frame": [H, W], "chroma": tag, "frame_bytes": fb, "blocks_per_plane": list(V.block_counts(H, W, layout)),
           "bytes_read_or_copied_and_written": 2 * n * fb, "those_bytes_at_the_copy_ceiling_ms": round(ideal, 4), "ms_per_call": ms}
    for k in calls:
        rec[k] = {"fraction_of_copy_ceiling": round(ideal / ms[k]["median"], 3), "over_the_copy": round(ms[k]["median"] / copy, 3)}
    rec["block_sad_over_plane_sse"] = round(ms["ssm_block_sad_fwd"]["median"] / ms["ssm_plane_sse_fwd"]["median"], 3)
    return rec


def bench_fps(dev, runs):
    import numpy as np
    from ssm_amd import video as V
    model, cfg = synthetic_model(dev)
    matrix, siting = V.default_matrix(H), V.CENTRED
    base = synthetic_payloads(BASE_FRAMES, H, W, dev, cfg)
    times = [2 + i % 2 for i in range(BASE_FRAMES)]          # 2, 3, 2, 3, ...
    repeated = np.repeat(base, times, axis=0)
    assert len(repeated) == 65
    acts, rep = V.dedup_host(repeated, H, W, siting)
    assert [r[1:3] for r in rep.log] == [(t - 1, True) for t in times[:-1]] + [(times[-1] - 1, False)], "the base clip moves: only the copies repeat"
    legs = ("dedup_upsample_rate_1_65_frames_720p", "upsample_rate_2_26_base_frames_720p")
    vis = dict(zip(legs, (V.VideoInterpolator(model, cfg, upsample_rate=1, n_streams=2, pairs_per_batch=1, matrix=matrix, dedup=True),
                          V.VideoInterpolator(model, cfg, upsample_rate=2, n_streams=2, pairs_per_batch=1, matrix=matrix))))
    count = {}
    with tempfile.TemporaryDirectory(prefix="bench_dedup_") as tmp:
        paths = dict(zip(legs, (os.path.join(tmp, "repeated.y4m"), os.path.join(tmp, "base.y4m"))))
        for name, clip in zip(legs, (repeated, base)):
            write_y4m(paths[name], clip, W, H, (60, 1))

        def run(name):          # the clock runs while the files are opened and closed
            t0 = time.perf_counter()
            with V.Y4MReader(paths[name]) as r:
                with V.Y4MWriter.like(os.devnull, r) as w:
                    count[name] = vis[name].run(r, w)
                    w.f.flush()
            return time.perf_counter() - t0

        secs = timed_legs(legs, run, runs)
    runs_log = vis[legs[0]].repeats
    assert count == {legs[0]: 65, legs[1]: 2 * BASE_FRAMES - 1} and len(runs_log) == BASE_FRAMES and sum(1 for r in runs_log if r[2]) == 25
    synthesised = {legs[0]: sum(t for t in times[:-1]) - 25, legs[1]: BASE_FRAMES - 1}
    return {"output_frames_per_s": {k: per_s(count[k], ts) for k, ts in secs.items()},
            "synthesised_frames_per_s": {k: per_s(synthesised[k], ts) for k, ts in secs.items()},
            "seconds_per_run": {k: [round(t, 3) for t in ts] for k, ts in secs.items()},
            "outputs": count, "synthesised": synthesised, "pairs_run": {k: BASE_FRAMES - 1 for k in legs},
            "runs_of_repeats": len(runs_log), "repaired": 25,
            "dedup_over_base_time_per_run": round(statistics.median(secs[legs[0]]) / statistics.median(secs[legs[1]]), 4),
            "note": "%d base frames of %dx%d repeated 2, 3, 2, 3, ... times as 65 frames through dedup=True, upsample_rate=1 (slots = 2), and "
                    "as they are through upsample_rate=2; file to /dev/null, 2 streams x 1 pair, legs in turns, %d timed runs each; both "
                    "legs run 25 pairs, the first synthesises 37 frames and reads, uploads and compares 65, the second synthesises 25"
                    % (BASE_FRAMES, W, H, runs)}


def run_step(step, args):
    import torch
    assert torch.cuda.is_available(), "bench_dedup.py measures on the GPU; there is no CPU path"
    dev = torch.device("cuda:0")
    return bench_fps(dev, args.runs) if step == "fps" else bench_kernel(dev, TAGS[step], args.iters, args.windows)


HEAD = ("Repair of repeated frames of the streamed video path (ssm_block_sad_fwd, RepeatSource, --dedup; DESIGN 3.12).\nOne MI355X, the "
        "default precision, synthetic weights and frames.  Tool: tools/bench_dedup.py (each step a process under its own time "
        "limit).\nNothing is asserted; with synthetic weights nothing can be said about quality.\n")


def main():
    args = parser("dedup_bench.txt", STEPS).parse_args()
    if args.only:
        return run_only(args.only, lambda: run_step(args.only, args))
    return drive(__file__, HEAD, STEPS, args)


if __name__ == "__main__":
    sys.exit(main())
