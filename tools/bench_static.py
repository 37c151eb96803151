"""Blocks that do not change of the streamed video path (ssm_amd/video.py) on synthetic frames.  Driver, timers and fixture are
tools/video_bench.py's: three steps, each a child process under its own `timeout`, chained - the first one that fails (or runs into its
limit) ends the run.  Each step prints one JSON line:
  kernel_bytes, kernel_words
           event-timed ssm_static_paste_fwd on 7 frame pairs (rows n against rows n + 1 of 8 payloads of 720 x 1280, 420jpeg or 422p10)
           with T = 7 outputs per pair, on a clip of random samples in which no block is static and on one in which the top left quarter
           of every frame is frame 0's (3600 of 14400 blocks static: the call then also writes 7 x a quarter of a frame per pair), beside
           ssm_block_sad_fwd on the same operands and a device-to-device copy of as many bytes as the calls READ, ALTERNATED in one run: a
           round times every call once, window after window.  Per call: the median over `--windows` rounds of `--iters` back-to-back
           calls, with the least and the largest; the bytes read as a fraction of the 6.29 TB/s copy ceiling (tools/bench_video.py).  The
           outputs and counts are checked against the yardstick first.
  fps      output frames per second of wall time, file to /dev/null, in turns on one box: a 65-frame 720 x 1280 clip (33 moving frames
           there and back) whose top left quarter is frame 0's, through VideoInterpolator(upsample_rate=8) with and without static=0 -
           64 pairs, 448 synthesised frames either way.
Nothing is asserted on the numbers.  With synthetic weights nothing can be said about quality.
Usage: python tools/bench_static.py [--out profiles/static_bench.txt] [--only STEP] [--iters 20] [--windows 7] [--runs 3]"""
import os
import statistics
import sys
import tempfile
import time

from video_bench import (COPY_CEILING_BYTES_PER_S, alternated_ms, drive, parser, per_s, run_only, synthetic_model, synthetic_payloads,
                         timed_legs, write_y4m)

STEPS = (("kernel_bytes", 180), ("kernel_words", 180), ("fps", 600))          # step, its time limit in seconds
H, W, BASE_FRAMES, T = 720, 1280, 33, 7
TAGS = {"kernel_bytes": "420jpeg", "kernel_words": "422p10"}


def keep_quarter(frames, layout, bits):
    """The top left quarter of every frame - 45 x 80 of the 90 x 160 blocks, luma and the chroma under them - becomes frame 0's."""
    from ssm_amd import video as V
    cr, cc = V._chroma_block(layout)
    for plane, (rr, rc) in zip(V.split_planes(frames, H, W, layout, bits), ((8, 8), (cr, cc), (cr, cc))):
        plane[1:, :45 * rr, :80 * rc] = plane[:1, :45 * rr, :80 * rc]
    return frames


def bench_kernel(dev, tag, iters, windows):
    import numpy as np
    import torch
    from ssm_amd import video as V
    n = 7
    layout, bits = V.EXTENDED_TAGS[tag]
    fb = V.frame_bytes(H, W, layout, bits)
    gen = torch.Generator(device="cpu").manual_seed(1)
    host = {"none": torch.randint(0, 256, (n + 1, fb), generator=gen, dtype=torch.uint8).numpy()}
    host["quarter"] = keep_quarter(host["none"].copy(), layout, bits)
    filler = torch.randint(0, 256, (n * T, fb), generator=gen, dtype=torch.uint8)
    frames = {k: torch.from_numpy(x).to(dev) for k, x in host.items()}
    out = torch.empty(n * T, fb, dtype=torch.uint8, device=dev)
    counts = torch.empty(n, dtype=torch.int64, device=dev)
    static = {}
    for k, f in frames.items():
        out.copy_(filler)
        V.static_paste(f[:-1], f[1:], out, H, W, layout, bits, 0, counts=counts)
        want, want_counts = V.static_paste_host(filler.numpy().reshape(n, T, fb), host[k][:-1], host[k][1:], H, W, layout, bits, 0)
        assert np.array_equal(out.cpu().numpy(), want.reshape(n * T, fb)) and counts.cpu().numpy().tolist() == want_counts.tolist()
        static[k] = int(want_counts[0])
    assert static == {"none": 0, "quarter": 3600}
    words = torch.empty(n, 3, 2, dtype=torch.int64, device=dev)
    src, dst = torch.empty(2 * n * fb, dtype=torch.uint8, device=dev).random_(), torch.empty(2 * n * fb, dtype=torch.uint8, device=dev)
    none, quarter = frames["none"], frames["quarter"]
    calls = {"ssm_static_paste_fwd_no_block_static": lambda: V.static_paste(none[:-1], none[1:], out, H, W, layout, bits, 0, counts=counts),
             "ssm_static_paste_fwd_a_quarter_static": lambda: V.static_paste(quarter[:-1], quarter[1:], out, H, W, layout, bits, 0, counts=counts),
             "ssm_block_sad_fwd": lambda: V.block_sad(none[1:], none[:-1], H, W, layout, bits, out=words),
             "d2d_copy_of_as_many_bytes_as_are_read": lambda: dst.copy_(src)}
    ms = alternated_ms(calls, iters, windows)
    copy = ms["d2d_copy_of_as_many_bytes_as_are_read"]["median"]
    ideal = 1e3 * 2 * n * fb / COPY_CEILING_BYTES_PER_S
    rec = {"pairs": n, "outputs_per_pair": T, "frame": [H, W], "chroma": tag, "frame_bytes": fb, "blocks": V.static_blocks(H, W),
           "static_blocks_per_pair": static, "bytes_read": 2 * n * fb, "bytes_written_a_quarter_static": n * T * fb // 4,
           "the_copy_reads_and_writes": 2 * n * fb, "bytes_read_at_the_copy_ceiling_ms": round(ideal, 4), "ms_per_call": ms}
    for k in calls:
        rec[k] = {"fraction_of_copy_ceiling": round(ideal / ms[k]["median"], 3), "over_the_copy": round(ms[k]["median"] / copy, 3)}
    rec["static_paste_over_block_sad"] = round(ms["ssm_static_paste_fwd_no_block_static"]["median"] / ms["ssm_block_sad_fwd"]["median"], 3)
    return rec


def bench_fps(dev, runs):
    import numpy as np
    from ssm_amd import video as V
    model, cfg = synthetic_model(dev)
    matrix, siting = V.default_matrix(H), V.CENTRED
    base = synthetic_payloads(BASE_FRAMES, H, W, dev, cfg)
    clip = keep_quarter(np.concatenate([base, base[-2::-1]]), siting, 8)          # there and back: 65 frames, neighbours always differ
    assert len(clip) == 65
    _, per_pair = V.static_paste_host(np.zeros((64, 1, clip.shape[1]), np.uint8), clip[:-1], clip[1:], H, W, siting, 8, 0)
    legs = ("static_0_upsample_rate_8_65_frames_720p", "upsample_rate_8_65_frames_720p")
    vis = dict(zip(legs, (V.VideoInterpolator(model, cfg, upsample_rate=8, n_streams=2, pairs_per_batch=1, matrix=matrix, static=0),
                          V.VideoInterpolator(model, cfg, upsample_rate=8, n_streams=2, pairs_per_batch=1, matrix=matrix))))
    count = {}
    with tempfile.TemporaryDirectory(prefix="bench_static_") as tmp:
        path = os.path.join(tmp, "clip.y4m")
        write_y4m(path, clip, W, H, (30, 1))

        def run(name):          # the clock runs while the files are opened and closed
            t0 = time.perf_counter()
            with V.Y4MReader(path) as r:
                with V.Y4MWriter.like(os.devnull, r) as w:
                    count[name] = vis[name].run(r, w)
                    w.f.flush()
            return time.perf_counter() - t0

        secs = timed_legs(legs, run, runs)
    kept = vis[legs[0]].static
    assert count == {k: 64 * 8 + 1 for k in legs} and [s for _, s, _ in kept] == per_pair.tolist() and vis[legs[1]].static == []
    med = {k: statistics.median(ts) for k, ts in secs.items()}
    return {"output_frames_per_s": {k: per_s(count[k], ts) for k, ts in secs.items()},
            "seconds_per_run": {k: [round(t, 3) for t in ts] for k, ts in secs.items()},
            "outputs": count, "pairs": 64, "synthesised": 448, "blocks": V.static_blocks(H, W),
            "static_blocks_per_pair": {"min": int(per_pair.min()), "max": int(per_pair.max())},
            "static_over_plain_time_per_run": round(med[legs[0]] / med[legs[1]], 4),
            "spread_of_the_plain_leg": round((max(secs[legs[1]]) - min(secs[legs[1]])) / med[legs[1]], 4),
            "note": "%d moving frames of %dx%d there and back as 65 frames, the top left quarter of every frame frame 0's, through "
                    "upsample_rate=8 with static=0 and without; file to /dev/null, 2 streams x 1 pair, legs in turns, %d timed runs each"
                    % (BASE_FRAMES, W, H, runs)}


def run_step(step, args):
    import torch
    assert torch.cuda.is_available(), "bench_static.py measures on the GPU; there is no CPU path"
    dev = torch.device("cuda:0")
    return bench_fps(dev, args.runs) if step == "fps" else bench_kernel(dev, TAGS[step], args.iters, args.windows)


HEAD = ("Blocks that do not change of the streamed video path (ssm_static_paste_fwd, --static; DESIGN 3.12).\nOne MI355X, the default "
        "precision, synthetic weights and frames.  Tool: tools/bench_static.py (each step a process under its own time limit).\n"
        "Nothing is asserted; with synthetic weights nothing can be said about quality.\n")


def main():
    args = parser("static_bench.txt", STEPS).parse_args()
    if args.only:
        return run_only(args.only, lambda: run_step(args.only, args))
    return drive(__file__, HEAD, STEPS, args)


if __name__ == "__main__":
    sys.exit(main())
