"""3:2 pulldown removal of the streamed video path (ssm_amd/video.py) on synthetic frames.  Driver, timers and fixture are
tools/video_bench.py's: three steps, each a child process under its own `timeout`, chained - the first one that fails (or runs into its
limit) ends the run.  Each step prints one JSON line:
  kernel_bytes, kernel_words
           event-timed ssm_field_diff_fwd on 7 frame pairs (rows n + 1 against rows n of 8 payloads of 720 x 1280, 4:2:0, 8-bit or 10-bit in
           words), beside a device-to-device copy of as many bytes as the call reads and, on the byte operands, ssm_luma_sad_fwd on the
           same pairs, ALTERNATED in one run: a round times every call once, window after window.  Per call: the median over `--windows`
           rounds of `--iters` back-to-back calls, with the least and the largest; the bytes the call reads as a fraction of the 6.29 TB/s
           copy ceiling (tools/bench_video.py).  The sums are checked against the yardsticks first.
  fps      output frames per second of wall time, file to /dev/null, in turns through ONE VideoInterpolator(upsample_rate=2): a 65-frame
           720 x 1280 telecined clip through TelecineSource (52 film frames, 103 outputs) beside the 52-frame film clip it was made from
           (the same 103 outputs): what the pulldown removal costs the stream.  A run of the first leg makes its TelecineSource, pinned
           buffers included.
Nothing is asserted on the numbers.  With synthetic weights nothing can be said about quality.
Usage: python tools/bench_detelecine.py [--out profiles/detelecine_bench.txt] [--only STEP] [--iters 20] [--windows 7] [--runs 3]"""
import os
import statistics
import sys
import tempfile
import time

from video_bench import (COPY_CEILING_BYTES_PER_S, alternated_ms, drive, parser, per_s, run_only, synthetic_model, synthetic_payloads,
                         timed_legs, write_y4m)

STEPS = (("kernel_bytes", 180), ("kernel_words", 180), ("fps", 600))          # step, its time limit in seconds
H, W, FILM_FRAMES = 720, 1280, 52
TAGS = {"kernel_bytes": "420jpeg", "kernel_words": "420p10"}


def bench_kernel(dev, tag, iters, windows):
    import numpy as np
    import torch
    from ssm_amd import video as V
    n = 7
    layout, bits = V.EXTENDED_TAGS[tag]
    fb, luma = V.frame_bytes(H, W, layout, bits), H * W * V.sample_bytes(bits)
    gen = torch.Generator(device="cpu").manual_seed(1)
    host = torch.randint(0, 256, (n + 1, fb), generator=gen, dtype=torch.uint8)
    frames = host.to(dev)
    new, old = frames[1:], frames[:-1]
    sums = torch.empty(n, 2, dtype=torch.int64, device=dev)
    V.field_diff(new, old, H, W, bits, out=sums)
    assert np.array_equal(sums.cpu().numpy().view(np.uint64), V.field_diff_host(host.numpy()[1:], host.numpy()[:-1], H, W, bits))
    src, dst = torch.empty(n * luma, dtype=torch.uint8, device=dev).random_(), torch.empty(n * luma, dtype=torch.uint8, device=dev)
    calls = {"ssm_field_diff_fwd": lambda: V.field_diff(new, old, H, W, bits, out=sums), "d2d_copy_of_as_many_bytes": lambda: dst.copy_(src)}
    if bits == 8:
        sad = torch.empty(n, dtype=torch.int64, device=dev)
        V.luma_sad(new, old, H, W, out=sad)
        y = host.numpy()[:, :luma].reshape(-1, H, W)
        assert np.array_equal(sad.cpu().numpy().view(np.uint64), V.luma_sad_host(y[1:], y[:-1]))
        assert np.array_equal(sums.cpu().numpy().sum(axis=1), sad.cpu().numpy()), "the two fields' differences add up to the plane's"
        calls["ssm_luma_sad_fwd"] = lambda: V.luma_sad(new, old, H, W, out=sad)
    ms = alternated_ms(calls, iters, windows)
    copy = ms["d2d_copy_of_as_many_bytes"]["median"]
    ideal = 1e3 * 2 * n * luma / COPY_CEILING_BYTES_PER_S
    rec = {"pairs": n, "frame": [H, W], "chroma": tag, "frame_bytes": fb, "bytes_read_or_copied_and_written": 2 * n * luma,
           "those_bytes_at_the_copy_ceiling_ms": round(ideal, 4), "ms_per_call": ms}
    for k in calls:
        rec[k] = {"fraction_of_copy_ceiling": round(ideal / ms[k]["median"], 3), "over_the_copy": round(ms[k]["median"] / copy, 3)}
    if bits == 8:
        rec["field_diff_over_luma_sad"] = round(ms["ssm_field_diff_fwd"]["median"] / ms["ssm_luma_sad_fwd"]["median"], 3)
    return rec


def bench_fps(dev, runs):
    from ssm_amd import video as V
    model, cfg = synthetic_model(dev)
    base = 43          # synthetic_frames_u8 holds 43 frames at the most: the film plays them forth and back
    matrix, siting = V.default_matrix(H), V.CENTRED
    made = synthetic_payloads(base, H, W, dev, cfg)
    period = 2 * (base - 1)
    film = made[[i % period if i % period < base else period - i % period for i in range(FILM_FRAMES)]]
    video = V.telecine_host(film, H, W, siting, 8, 0, 0)
    assert len(video) == 65
    rate = (30000, 1001)
    vi = V.VideoInterpolator(model, cfg, upsample_rate=2, n_streams=2, pairs_per_batch=1, matrix=matrix)
    legs = ("detelecine_upsample_rate_2_65_frames_720p", "upsample_rate_2_52_film_frames_720p")
    count, cadence = {}, {}
    with tempfile.TemporaryDirectory(prefix="bench_detelecine_") as tmp:
        paths = dict(zip(legs, (os.path.join(tmp, "telecined.y4m"), os.path.join(tmp, "film.y4m"))))
        for name, clip, r in zip(legs, (video, film), (rate, V.detelecine_rate(rate))):
            write_y4m(paths[name], clip, W, H, r)

        def run(name):          # the clock runs while the files are opened and closed and the TelecineSource is made
            t0 = time.perf_counter()
            with V.Y4MReader(paths[name], interlaced=True) as r:
                if name == legs[0]:
                    r = V.TelecineSource(r, dev)
                with V.Y4MWriter.like(os.devnull, r, rate=V.output_rate(r.rate, 2)) as w:
                    count[name] = vi.run(r, w)
                    w.f.flush()
            dt = time.perf_counter() - t0
            if name == legs[0]:
                cadence.update(windows=len(r.cadence), hypotheses=sorted({h for _, h, _, _ in r.cadence}), dropped=r.dropped)
            return dt

        secs = timed_legs(legs, run, runs)
    assert count == {k: 2 * FILM_FRAMES - 1 for k in legs} and cadence == {"windows": 12, "hypotheses": [0], "dropped": 13}
    return {"output_frames_per_s": {k: per_s(count[k], ts) for k, ts in secs.items()},
            "seconds_per_run": {k: [round(t, 3) for t in ts] for k, ts in secs.items()},
            "outputs": count, "cadence": cadence,
            "detelecine_over_film_time_per_run": round(statistics.median(secs[legs[0]]) / statistics.median(secs[legs[1]]), 4),
            "note": "%d film frames of %dx%d (43 synthetic frames forth and back) in 3:2 pulldown as 65 video frames, and as they are; file to "
                    "/dev/null, one VideoInterpolator, 2 streams x 1 pair, legs in turns, %d timed runs each; a run opens its file and, the "
                    "first leg, makes its TelecineSource" % (FILM_FRAMES, W, H, runs)}


def run_step(step, args):
    import torch
    assert torch.cuda.is_available(), "bench_detelecine.py measures on the GPU; there is no CPU path"
    dev = torch.device("cuda:0")
    return bench_fps(dev, args.runs) if step == "fps" else bench_kernel(dev, TAGS[step], args.iters, args.windows)


HEAD = ("3:2 pulldown removal of the streamed video path (ssm_field_diff_fwd, TelecineSource, --detelecine; DESIGN 3.12).\nOne MI355X, the "
        "default precision, synthetic weights and frames.  Tool: tools/bench_detelecine.py (each step a process under its own time "
        "limit).\nNothing is asserted; with synthetic weights nothing can be said about quality.\n")


def main():
    args = parser("detelecine_bench.txt", STEPS).parse_args()
    if args.only:
        return run_only(args.only, lambda: run_step(args.only, args))
    return drive(__file__, HEAD, STEPS, args)


if __name__ == "__main__":
    sys.exit(main())
