"""Letterboxed clips of the streamed video path (ssm_amd/video.py) on synthetic frames.  Driver, timers and fixture are
tools/video_bench.py's: three steps, each a child process under its own `timeout`, chained - the first one that fails (or runs into its
limit) ends the run.  Each step prints one JSON line:
  kernel_bytes, kernel_words
           event-timed ssm_luma_counts_fwd and ssm_window_cut_fwd (the 1920 x 800 picture at row 140) on 7 frames of 1080 x 1920, 420jpeg
           or 422p10, beside ssm_luma_sad_fwd on the same bytes (frames n + 1 against n; in 422p10 its bytes are the low and high halves
           of the words, which it reads all the same) and a device-to-device copy of as many bytes as 7 frames hold, ALTERNATED in one
           run: a round times every call once, window after window.  Per call: the median over `--windows` rounds of `--iters`
           back-to-back calls, with the least and the largest, and its ratio to the copy and to ssm_luma_sad_fwd.  Counts and windows are
           checked against the yardsticks first.
  fps      output frames per second of wall time, file to /dev/null, in turns on one box, at upsample_rate 8: a 65-frame 1080 x 1920 clip
           with a 1920 x 800 picture through VideoInterpolator(active="auto"), the same clip without the option, and the 1920 x 800 clip
           alone.  with_active over alone is the cost of cut, paste and probe; with_active over without is what the option saves.
Nothing is asserted on the numbers.  With synthetic weights nothing can be said about quality.
Usage: python tools/bench_active.py [--out profiles/active_bench.txt] [--only STEP] [--iters 20] [--windows 7] [--runs 3]"""
import os
import statistics
import sys
import tempfile
import time

from video_bench import alternated_ms, drive, parser, per_s, run_only, synthetic_model, synthetic_payloads, timed_legs, write_y4m

STEPS = (("kernel_bytes", 180), ("kernel_words", 180), ("fps", 900))          # step, its time limit in seconds
H, W, FRAMES = 1080, 1920, 65
RECT = (1920, 800, 0, 140)          # (w, h, x, y): a 2.40:1 picture
TAGS = {"kernel_bytes": "420jpeg", "kernel_words": "422p10"}


def bench_kernel(dev, tag, iters, windows):
    import numpy as np
    import torch
    from ssm_amd import video as V
    n = 7
    layout, bits = V.EXTENDED_TAGS[tag]
    fb, wb = V.frame_bytes(H, W, layout, bits), V.frame_bytes(RECT[1], RECT[0], layout, bits)
    gen = torch.Generator(device="cpu").manual_seed(1)
    host = torch.randint(0, 256, (n + 1, fb), generator=gen, dtype=torch.uint8)
    if bits > 8:
        host.numpy().view("<u2")[...] &= (1 << bits) - 1
    frames = host.to(dev)
    rows, cols = torch.empty(n, H, dtype=torch.int32, device=dev), torch.empty(n, W, dtype=torch.int32, device=dev)
    limit = (1 << bits) // 2
    V.luma_counts(frames[:n], H, W, bits, limit, rows, cols)
    want = V.active_counts_host(host.numpy()[:n], H, W, bits, limit)
    assert np.array_equal(rows.cpu().numpy().view(np.uint32), want[0]) and np.array_equal(cols.cpu().numpy().view(np.uint32), want[1])
    wins = torch.empty(n, wb, dtype=torch.uint8, device=dev)
    V.window_cut(frames[:n], H, W, layout, bits, RECT, out=wins)
    assert np.array_equal(wins.cpu().numpy(), V.cut_window_host(host.numpy()[:n], H, W, layout, bits, RECT))
    sb = V.sample_bytes(bits)
    sad = torch.empty(n, dtype=torch.int64, device=dev)
    src, dst = torch.empty(n * fb, dtype=torch.uint8, device=dev).random_(), torch.empty(n * fb, dtype=torch.uint8, device=dev)
    calls = {"ssm_luma_counts_fwd": lambda: V.luma_counts(frames[:n], H, W, bits, limit, rows, cols),
             "ssm_window_cut_fwd": lambda: V.window_cut(frames[:n], H, W, layout, bits, RECT, out=wins),
             "ssm_luma_sad_fwd": lambda: V.luma_sad(frames[1:], frames[:-1], H, W * sb, out=sad),
             "d2d_copy_of_7_frames": lambda: dst.copy_(src)}
    ms = alternated_ms(calls, iters, windows)
    copy, lsad = ms["d2d_copy_of_7_frames"]["median"], ms["ssm_luma_sad_fwd"]["median"]
    rec = {"frames": n, "frame": [H, W], "window_w_h_x_y": list(RECT), "chroma": tag, "frame_bytes": fb, "window_bytes": wb,
           "bytes": {"ssm_luma_counts_fwd reads": n * H * W * sb, "ssm_window_cut_fwd reads and writes": 2 * n * wb,
                     "ssm_luma_sad_fwd reads": 2 * n * H * W * sb, "d2d_copy_of_7_frames reads and writes": 2 * n * fb},
           "ms_per_call": ms}
    for k in calls:
        rec[k] = {"over_the_copy_of_7_frames": round(ms[k]["median"] / copy, 3), "over_luma_sad": round(ms[k]["median"] / lsad, 3)}
    return rec


def bench_fps(dev, runs):
    import numpy as np
    from ssm_amd import video as V
    model, cfg = synthetic_model(dev)
    pw, ph = RECT[:2]
    matrix, siting = V.default_matrix(H), V.CENTRED          # the picture's 800 rows get the frame's matrix either way
    half = FRAMES // 2 + 1          # the synthetic clip moves (3, 2) pixels a frame and has room for 42 frames: there and back again
    picture = synthetic_payloads(half, ph, pw, dev, cfg)
    picture = np.concatenate([picture, picture[-2::-1]])
    assert len(picture) == FRAMES
    bars = np.zeros((FRAMES, V.frame_bytes(H, W, siting)), np.uint8)
    y, u, v = V.split_planes(bars, H, W, siting)
    y[...], u[...], v[...] = 16, 128, 128
    boxed = V.paste_window_host(picture, bars, H, W, siting, 8, RECT, out=bars)
    assert V.active_area_host(boxed, H, W, siting)[0] == RECT
    legs = ("with_active_auto_1080p", "without_active_1080p", "picture_alone_800p")
    kw = dict(upsample_rate=8, n_streams=2, pairs_per_batch=1, matrix=matrix)
    vis = dict(zip(legs, (V.VideoInterpolator(model, cfg, active="auto", **kw), V.VideoInterpolator(model, cfg, **kw),
                          V.VideoInterpolator(model, cfg, **kw))))
    count, turns = {}, []
    with tempfile.TemporaryDirectory(prefix="bench_active_") as tmp:
        paths = dict(zip(legs, (os.path.join(tmp, "boxed.y4m"), os.path.join(tmp, "boxed.y4m"), os.path.join(tmp, "picture.y4m"))))
        for name, clip, (h, w) in ((legs[0], boxed, (H, W)), (legs[2], picture, (ph, pw))):
            write_y4m(paths[name], clip, w, h, (24, 1))

        def run(name):          # the clock runs while the files are opened and closed
            t0 = time.perf_counter()
            with V.Y4MReader(paths[name]) as r:
                with V.Y4MWriter.like(os.devnull, r) as w:
                    count[name] = vis[name].run(r, w)
                    w.f.flush()
            dt = time.perf_counter() - t0
            print("turn %d, %s: %.2f s" % (turns[-1], name, dt), file=sys.stderr, flush=True)
            return dt

        secs = timed_legs(legs, run, runs, between=turns.append)
    assert vis[legs[0]].active == RECT and vis[legs[0]].active_excess == [] and len(set(count.values())) == 1
    med = {k: statistics.median(ts) for k, ts in secs.items()}
    hp, wp = vis[legs[0]].canvas(ph, pw), vis[legs[0]].canvas(H, W)
    return {"output_frames_per_s": {k: per_s(count[k], ts) for k, ts in secs.items()},
            "seconds_per_run": {k: [round(t, 3) for t in ts] for k, ts in secs.items()},
            "outputs": count, "canvas": {"picture": list(hp), "frame": list(wp), "pixels_ratio": round(hp[0] * hp[1] / (wp[0] * wp[1]), 4)},
            "with_active_over_without_time_per_run": round(med[legs[0]] / med[legs[1]], 4),
            "with_active_over_picture_alone_time_per_run": round(med[legs[0]] / med[legs[2]], 4),
            "note": "%d frames of %dx%d with a %dx%d picture at row %d, upsample_rate 8, 420jpeg; file to /dev/null, 2 streams x 1 pair, legs in "
                    "turns, %d timed runs each; the first leg probes %d frames, cuts every uploaded frame on the GPU and pastes %d "
                    "synthesised windows on the writer thread" % (FRAMES, W, H, pw, ph, RECT[3], runs, min(FRAMES, 48), (FRAMES - 1) * 7)}


def run_step(step, args):
    import torch
    assert torch.cuda.is_available(), "bench_active.py measures on the GPU; there is no CPU path"
    dev = torch.device("cuda:0")
    return bench_fps(dev, args.runs) if step == "fps" else bench_kernel(dev, TAGS[step], args.iters, args.windows)


HEAD = ("Letterboxed clips of the streamed video path (ssm_luma_counts_fwd, ssm_window_cut_fwd, ActiveSource, --active; DESIGN 3.12).\nOne "
        "MI355X, the default precision, synthetic weights and frames.  Tool: tools/bench_active.py (each step a process under its own "
        "time limit).\nNothing is asserted; with synthetic weights nothing can be said about quality.\n")


def main():
    args = parser("active_bench.txt", STEPS).parse_args()
    if args.only:
        return run_only(args.only, lambda: run_step(args.only, args))
    return drive(__file__, HEAD, STEPS, args)


if __name__ == "__main__":
    sys.exit(main())
