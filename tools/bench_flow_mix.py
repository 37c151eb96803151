"""The per-block fallback as a cross-fade of the streamed video path (ssm_flow_mix_fwd, --flow_fallback mix; ssm_amd/video.py, DESIGN
3.12) on synthetic masks and frames, beside the nearer-frame fallback it stands in for.  Driver, timers and fixture are
tools/video_bench.py's: the steps are child processes under their own `timeout`, chained - the first one that fails (or runs into its
limit) ends the run.  Each step prints one JSON line:
  kernel_420jpeg / event-timed ssm_flow_mix_fwd on 7 pairs of 720 x 1280 with T = 7 outputs a pair (the fixed grid of upsample_rate 8:
  kernel_422p10    k_j = 1 + j over 8) against masks with no failed block, with a quarter failed and with all failed, beside
                   ssm_flow_paste_fwd on the same operands and masks (split = 3) and a device-to-device copy of the masks plus both
                   payloads, ALTERNATED in one run.  Per call: the median over `--windows` rounds of `--iters` back-to-back calls, with
                   the least and the largest; mix over nearer per mask, and beside it the ratio of the bytes the two move when every
                   block fails (1: at 0 < split < T nearer reads both payloads too) - the expectation is that the time ratio lies
                   between 1 and that; the record says whether it does.
                   Outputs and counts are checked against the yardstick first, on one pair.
  fps              output frames per second of wall time, file to /dev/null, in turns on one box: the 65-frame 720 x 1280 clip of
                   bench_flow_repair.py through VideoInterpolator(upsample_rate=8, flow_check=True, flow_blocks=63) with the fallback
                   nearer and with mix; after the first turn both interpolators run on the same HIP streams (video_bench.share_streams:
                   which hardware queues a pipeline's streams are dealt moves a leg by more than one launch a pass does).
  headline         `bench.py --gpus 1 --steps 20 --warmup 5` of this tree and, with --parent DIR (a built checkout of the parent commit),
                   of that tree, in turns, twice each, every run a process under its own time limit: the lines as they were printed.
Nothing is asserted on the numbers.  With synthetic weights nothing can be said about quality.
Usage: python tools/bench_flow_mix.py [--out profiles/flow_mix_bench.txt] [--only STEP] [--iters 20] [--windows 7] [--runs 3]
                                      [--parent DIR]"""
import os
import statistics
import sys
import tempfile
import time

from video_bench import (alternated_ms, drive, parser, per_s, run_only, share_streams, synthetic_model, synthetic_payloads, timed_legs,
                         write_y4m)

STEPS = (("kernel_420jpeg", 240), ("kernel_422p10", 240), ("fps", 600), ("headline", 1500))          # step, its time limit in seconds
H, W, BASE_FRAMES, PAIRS, T, SPLIT, MIX, K_FPS = 720, 1280, 33, 7, 7, 3, (1, 1, 8), 63


def bench_kernel(dev, tag, iters, windows):
    import numpy as np
    import torch
    from ssm_amd import video as V
    layout, bits = V.EXTENDED_TAGS[tag]
    fb, blocks = V.frame_bytes(H, W, layout, bits), V.static_blocks(H, W)
    rng = np.random.RandomState(3)
    frames = rng.randint(0, 256, size=(PAIRS + 1, fb)).astype(np.uint8)
    if bits > 8:
        frames.view("<u2")[...] &= (1 << bits) - 1
    fail = {"no_block_fails": np.zeros((PAIRS, H >> 3, W >> 3), bool), "a_quarter_fails": rng.rand(PAIRS, H >> 3, W >> 3) < 0.25,
            "every_block_fails": np.ones((PAIRS, H >> 3, W >> 3), bool)}
    masks = {}
    for name, f in fail.items():          # a failed block: all 64 pixels inconsistent in direction 0; every other pixel leaves (byte 2)
        m = np.full((PAIRS, 2, H, W), 2, np.uint8)
        m[:, 0] = np.where(np.repeat(np.repeat(f, 8, axis=1), 8, axis=2), 1, 2)
        masks[name] = m
    dev_frames = torch.from_numpy(frames).to(dev)
    a, b = dev_frames[:-1], dev_frames[1:]
    out = torch.empty(PAIRS * T, fb, dtype=torch.uint8, device=dev).random_()
    counts = torch.empty(PAIRS, dtype=torch.int64, device=dev)
    dev_masks = {k: torch.from_numpy(m).to(dev) for k, m in masks.items()}
    # the check, on one pair
    before = out[:T].cpu().numpy()
    V.flow_mix(a[:1], b[:1], out[:T], dev_masks["a_quarter_fails"][:1], H, W, layout, bits, 32, *MIX, counts=counts[:1])
    want, want_counts = V.flow_mix_host(before[None], frames[:1], frames[1:2], masks["a_quarter_fails"][:1], H, W, layout, bits, 32, *MIX)
    assert np.array_equal(out[:T].cpu().numpy(), want[0]) and counts[:1].cpu().numpy().tolist() == want_counts.tolist()
    nbytes = PAIRS * (2 * H * W + 2 * fb)
    src, dst = torch.empty(nbytes, dtype=torch.uint8, device=dev).random_(), torch.empty(nbytes, dtype=torch.uint8, device=dev)
    calls = {}
    for k, m in dev_masks.items():          # mix and nearer side by side on every mask, then the copy: one round times each once
        calls["ssm_flow_mix_fwd_" + k] = lambda m=m: V.flow_mix(a, b, out, m, H, W, layout, bits, 32, *MIX, counts=counts)
        calls["ssm_flow_paste_fwd_" + k] = lambda m=m: V.flow_paste(a, b, out, m, H, W, layout, bits, 32, SPLIT, counts=counts)
    calls["d2d_copy_of_masks_and_payloads"] = lambda: dst.copy_(src)
    ms = alternated_ms(calls, iters, windows)
    # every block fails: both kernels read the masks and BOTH payloads once (nearer with 0 < split < T takes a for its left outputs and b for
    # its right ones) and write the same T outputs, so the bytes moved are the same and the ratio of bytes is 1
    mask_bytes, side_bytes, out_bytes = PAIRS * 2 * H * W, PAIRS * fb, PAIRS * T * fb
    moved = mask_bytes + 2 * side_bytes + out_bytes
    ratio = {k: round(ms["ssm_flow_mix_fwd_" + k]["median"] / ms["ssm_flow_paste_fwd_" + k]["median"], 3) for k in dev_masks}
    bytes_ratio = 1.0
    all_fail = ratio["every_block_fails"]
    rec = {"pairs": PAIRS, "frame": [H, W], "format": tag, "outputs_per_pair": T, "split_of_nearer": SPLIT, "num0_num_step_den_of_mix": list(MIX),
           "blocks_per_frame": blocks, "mask_bytes": mask_bytes, "payload_bytes_of_both_sides": 2 * side_bytes, "the_copy_reads_and_writes": nbytes,
           "output_bytes_written_when_every_block_fails": out_bytes, "failed_blocks": {k: int(f.sum()) for k, f in fail.items()},
           "bytes_moved_by_either_when_every_block_fails": moved, "ms_per_call": ms, "mix_over_nearer": ratio,
           "mix_over_nearer_in_bytes_moved_when_every_block_fails": bytes_ratio,
           "mix_over_the_copy": {k: round(ms["ssm_flow_mix_fwd_" + k]["median"] / ms["d2d_copy_of_masks_and_payloads"]["median"], 3) for k in dev_masks},
           "expectation": "with 0 < split < T nearer reads both payloads too, so the bytes moved are the same and the expected range of mix "
                          "over nearer, 1 .. %.3f, is a point; mix adds two multiplies and a multiply-shift division per sample, so a time ratio above 1 at equal bytes may be "
                          "the arithmetic's and need be no anomaly - which of the two holds the kernel was not traced" % bytes_ratio}
    rec["every_block_fails_mix_over_nearer_lies"] = ("inside 1 .. %.3f" % bytes_ratio if 1 <= all_fail <= bytes_ratio else
                                                     "OUTSIDE 1 .. %.3f at %.3f; the kernel was not traced" % (bytes_ratio, all_fail))
    return rec


def bench_fps(dev, runs):
    import numpy as np
    from ssm_amd import video as V
    model, cfg = synthetic_model(dev)
    matrix = V.default_matrix(H)
    base = synthetic_payloads(BASE_FRAMES, H, W, dev, cfg)
    clip = np.concatenate([base, base[-2::-1]])          # there and back: 65 frames, neighbours always differ
    assert len(clip) == 65
    legs = ("flow_blocks_63_nearer_upsample_rate_8_65_frames_720p", "flow_blocks_63_mix_upsample_rate_8_65_frames_720p")
    kw = dict(upsample_rate=8, n_streams=2, pairs_per_batch=1, matrix=matrix, flow_check=True, flow_blocks=K_FPS)
    vis = dict(zip(legs, (V.VideoInterpolator(model, cfg, flow_fallback="nearer", **kw), V.VideoInterpolator(model, cfg, flow_fallback="mix", **kw))))
    count = {}
    with tempfile.TemporaryDirectory(prefix="bench_flow_mix_") as tmp:
        path = os.path.join(tmp, "clip.y4m")
        write_y4m(path, clip, W, H, (30, 1))

        def run(name):          # the clock runs while the files are opened and closed
            t0 = time.perf_counter()
            with V.Y4MReader(path) as r:
                with V.Y4MWriter.like(os.devnull, r) as w:
                    count[name] = vis[name].run(r, w)
                    w.f.flush()
            return time.perf_counter() - t0

        secs = timed_legs(legs, run, runs, warmup=2, between=share_streams(list(vis.values())))          # the legs differ by one launch a pass
    repaired = vis[legs[1]].flow_repaired
    assert count == {x: 64 * 8 + 1 for x in legs} and [i for i, _, _ in repaired] == list(range(64)) and vis[legs[0]].flow_repaired == repaired
    med = {x: statistics.median(ts) for x, ts in secs.items()}
    failed, of = sum(f for _, f, _ in repaired), sum(b for _, _, b in repaired)
    shares = [f / b for _, f, b in repaired]
    return {"output_frames_per_s": {x: per_s(count[x], ts) for x, ts in secs.items()},
            "seconds_per_run": {x: [round(t, 3) for t in ts] for x, ts in secs.items()},
            "outputs": count, "pairs": 64, "synthesised": 448, "K": K_FPS,
            "blocks_mixed_or_replaced": {"failed": failed, "of": of, "share": round(failed / of, 4), "largest_share_of_a_pair": round(max(shares), 4),
                                         "smallest_share_of_a_pair": round(min(shares), 4)},
            "mix_over_nearer_time_per_run": round(med[legs[1]] / med[legs[0]], 4),
            "spread_of_the_nearer_leg": round((max(secs[legs[0]]) - min(secs[legs[0]])) / med[legs[0]], 4),
            "note": "%d moving frames of %dx%d there and back as 65 frames through upsample_rate=8 with flow_check=True and flow_blocks=%d, "
                    "the fallback nearer and mix; file to /dev/null, 2 streams x 1 pair (the same HIP streams for both legs), legs in turns, %d timed runs each"
                    % (BASE_FRAMES, W, H, K_FPS, runs)}


def run_step(step, args):
    if step == "headline":
        from bench_flow_repair import bench_headline          # bench.py's line of two trees in turns: the same step, the same limits
        return bench_headline(args.parent)
    import torch
    assert torch.cuda.is_available(), "bench_flow_mix.py measures on the GPU; there is no CPU path"
    dev = torch.device("cuda:0")
    return bench_fps(dev, args.runs) if step == "fps" else bench_kernel(dev, step[len("kernel_"):], args.iters, args.windows)


HEAD = ("The per-block fallback as a cross-fade of the streamed video path (ssm_flow_mix_fwd, --flow_fallback mix; DESIGN 3.12).\nOne MI355X, the "
        "default precision, synthetic weights, masks and frames.  Tool: tools/bench_flow_mix.py (each step a process under its own time "
        "limit).\nNothing is asserted; with synthetic weights nothing can be said about quality.  No kernel trace was taken.\n")


def main():
    ap = parser("flow_mix_bench.txt", STEPS)
    ap.add_argument("--parent", default="", help="a built checkout of the parent commit, for the headline step")
    args = ap.parse_args()
    if args.only:
        return run_only(args.only, lambda: run_step(args.only, args))
    return drive(__file__, HEAD, STEPS, args)


if __name__ == "__main__":
    sys.exit(main())
