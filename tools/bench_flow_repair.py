"""The flow check's per-block fallback of the streamed video path (ssm_flow_paste_fwd, --flow_blocks; ssm_amd/video.py) on
synthetic masks and frames.  Driver, timers and fixture are tools/video_bench.py's: the steps are child processes under their own
`timeout`, chained - the first one that fails (or runs into its limit) ends the run.  Each step prints one JSON line:
  kernel_420jpeg / event-timed ssm_flow_paste_fwd on 7 pairs of 720 x 1280 with T = 7 outputs a pair (split = 3, the fixed grid of
  kernel_422p10    upsample_rate 8) against masks with no failed block, with a quarter failed and with all failed, beside
                   ssm_static_paste_fwd on the same payloads (lo = 0: a != b, so it reads both frames and keeps nothing) and a
                   device-to-device copy of the bytes the paste reads when every block fails (masks + both payloads), ALTERNATED in one
                   run.  Per call: the median over `--windows` rounds of `--iters` back-to-back calls, with the least and the largest;
                   the ratios to the copy and to the sibling.  Outputs and counts are checked against the yardstick first, on one pair.
  fps              output frames per second of wall time, file to /dev/null, in turns on one box: the 65-frame 720 x 1280 clip of
                   bench_static.py / bench_flow_check.py through VideoInterpolator(upsample_rate=8, flow_check=True) without and with
                   flow_blocks=K, K the median n of the blocks of eight of the clip's pairs (about half the blocks fail; stated).
  headline         `bench.py --gpus 1 --steps 20 --warmup 5` of this tree and, with --parent DIR (a built checkout of the parent commit),
                   of that tree, in turns, twice each, every run a process under its own time limit: the lines as they were printed.
Nothing is asserted on the numbers.  With synthetic weights nothing can be said about quality.
Usage: python tools/bench_flow_repair.py [--out profiles/flow_repair_bench.txt] [--only STEP] [--iters 20] [--windows 7] [--runs 3]
                                         [--parent DIR]"""
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

from video_bench import (COPY_CEILING_BYTES_PER_S, ROOT, alternated_ms, drive, parser, per_s, run_only, synthetic_model, synthetic_payloads,
                         timed_legs, write_y4m)

STEPS = (("kernel_420jpeg", 240), ("kernel_422p10", 240), ("fps", 600), ("headline", 1500))          # step, its time limit in seconds
H, W, BASE_FRAMES, PAIRS, T, SPLIT = 720, 1280, 33, 7, 7, 3
BENCH_LIMIT = 340          # one bench.py run, in seconds


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
    V.flow_paste(a[:1], b[:1], out[:T], dev_masks["a_quarter_fails"][:1], H, W, layout, bits, 32, SPLIT, counts=counts[:1])
    want, want_counts = V.flow_paste_host(before[None], frames[:1], frames[1:2], masks["a_quarter_fails"][:1], H, W, layout, bits, 32, SPLIT)
    assert np.array_equal(out[:T].cpu().numpy(), want[0]) and counts[:1].cpu().numpy().tolist() == want_counts.tolist()
    nbytes = PAIRS * (2 * H * W + 2 * fb)
    src, dst = torch.empty(nbytes, dtype=torch.uint8, device=dev).random_(), torch.empty(nbytes, dtype=torch.uint8, device=dev)
    calls = {"ssm_flow_paste_fwd_" + k: (lambda m=m: V.flow_paste(a, b, out, m, H, W, layout, bits, 32, SPLIT, counts=counts))
             for k, m in dev_masks.items()}
    calls["ssm_static_paste_fwd_lo_0_nothing_kept"] = lambda: V.static_paste(a, b, out, H, W, layout, bits, 0, counts=counts)
    calls["d2d_copy_of_masks_and_payloads"] = lambda: dst.copy_(src)
    ms = alternated_ms(calls, iters, windows)
    copy, sibling = ms["d2d_copy_of_masks_and_payloads"]["median"], ms["ssm_static_paste_fwd_lo_0_nothing_kept"]["median"]
    rec = {"pairs": PAIRS, "frame": [H, W], "format": tag, "outputs_per_pair": T, "split": SPLIT, "blocks_per_frame": blocks,
           "mask_bytes": PAIRS * 2 * H * W, "payload_bytes_of_both_sides": PAIRS * 2 * fb, "the_copy_reads_and_writes": nbytes,
           "output_bytes_written_when_every_block_fails": PAIRS * T * fb,
           "failed_blocks": {k: int(f.sum()) for k, f in fail.items()},
           "the_copy_at_the_copy_ceiling_ms": round(1e3 * nbytes / COPY_CEILING_BYTES_PER_S, 4), "ms_per_call": ms}
    for k in calls:
        rec[k] = {"over_the_copy": round(ms[k]["median"] / copy, 3), "over_the_sibling": round(ms[k]["median"] / sibling, 3)}
    return rec


def bench_fps(dev, runs):
    import numpy as np
    import torch
    from ssm_amd import video as V
    model, cfg = synthetic_model(dev)
    matrix = V.default_matrix(H)
    base = synthetic_payloads(BASE_FRAMES, H, W, dev, cfg)
    clip = np.concatenate([base, base[-2::-1]])          # there and back: 65 frames, neighbours always differ
    assert len(clip) == 65
    # K: the median n over the blocks of eight pairs of the clip, from the masks of FullModel.flow_consistency on the frames as the loop
    # ingests them - about half the blocks have more
    picks = list(range(0, 64, 8))
    planes = V.frames_from_yuv(torch.from_numpy(clip).to(dev), H, W, V.CENTRED, matrix, V.LIMITED, cfg, True)
    n_blocks = []
    for i in picks:
        _, mask = model.flow_consistency(torch.stack([planes[i], planes[i + 1]])[None], size=(H, W), want_mask=True)
        n_blocks.append(V.flow_block_counts_host(mask.cpu().numpy(), H, W).reshape(-1))
    n_blocks = np.concatenate(n_blocks)
    del planes
    k = min(int(np.median(n_blocks)), 63)
    legs = ("flow_check_upsample_rate_8_65_frames_720p", "flow_check_flow_blocks_upsample_rate_8_65_frames_720p")
    kw = dict(upsample_rate=8, n_streams=2, pairs_per_batch=1, matrix=matrix, flow_check=True)
    vis = dict(zip(legs, (V.VideoInterpolator(model, cfg, **kw), V.VideoInterpolator(model, cfg, flow_blocks=k, **kw))))
    count = {}
    with tempfile.TemporaryDirectory(prefix="bench_flow_repair_") as tmp:
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
    repaired = vis[legs[1]].flow_repaired
    assert count == {x: 64 * 8 + 1 for x in legs} and [i for i, _, _ in repaired] == list(range(64)) and vis[legs[0]].flow_repaired == []
    med = {x: statistics.median(ts) for x, ts in secs.items()}
    failed, of = sum(f for _, f, _ in repaired), sum(b for _, _, b in repaired)
    shares = [f / b for _, f, b in repaired]
    return {"output_frames_per_s": {x: per_s(count[x], ts) for x, ts in secs.items()},
            "seconds_per_run": {x: [round(t, 3) for t in ts] for x, ts in secs.items()},
            "outputs": count, "pairs": 64, "synthesised": 448, "K": k,
            "n_of_the_blocks_of_pairs": {"pairs": picks, "min": int(n_blocks.min()), "median": float(np.median(n_blocks)), "max": int(n_blocks.max())},
            "blocks_replaced": {"failed": failed, "of": of, "share": round(failed / of, 4), "largest_share_of_a_pair": round(max(shares), 4),
                                "smallest_share_of_a_pair": round(min(shares), 4)},
            "flow_blocks_over_flow_check_time_per_run": round(med[legs[1]] / med[legs[0]], 4),
            "spread_of_the_flow_check_leg": round((max(secs[legs[0]]) - min(secs[legs[0]])) / med[legs[0]], 4),
            "note": "%d moving frames of %dx%d there and back as 65 frames through upsample_rate=8 with flow_check=True, without and with "
                    "flow_blocks=K; file to /dev/null, 2 streams x 1 pair, legs in turns, %d timed runs each" % (BASE_FRAMES, W, H, runs)}


def bench_headline(parent):
    """bench.py's line of this tree and of `parent`, in turns; every run a process of its own under BENCH_LIMIT.  This process opens no GPU."""
    trees = [("this_commit", ROOT)] + ([("parent_commit", os.path.abspath(parent))] if parent else [])
    lines = {name: [] for name, _ in trees}
    for _ in range(2):
        for name, root in trees[::-1]:
            r = subprocess.run(["timeout", "-k", "10", str(BENCH_LIMIT), sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "20",
                                "--warmup", "5"], cwd=root, stdout=subprocess.PIPE, text=True)
            if r.returncode != 0:          # a failure, a fault or a time limit: nothing more is started
                raise SystemExit(r.returncode)
            lines[name].append(json.loads(r.stdout.strip().splitlines()[-1]))
    rec = {"command": "bench.py --gpus 1 --steps 20 --warmup 5", "order": "parent, this, parent, this" if parent else "this, this", "lines": lines}
    if not parent:
        rec["parent_commit"] = "not measured: no --parent tree was given"
    return rec


def run_step(step, args):
    if step == "headline":
        return bench_headline(args.parent)
    import torch
    assert torch.cuda.is_available(), "bench_flow_repair.py measures on the GPU; there is no CPU path"
    dev = torch.device("cuda:0")
    return bench_fps(dev, args.runs) if step == "fps" else bench_kernel(dev, step[len("kernel_"):], args.iters, args.windows)


HEAD = ("The flow check's per-block fallback of the streamed video path (ssm_flow_paste_fwd, --flow_blocks; DESIGN 3.12).\nOne MI355X, the "
        "default precision, synthetic weights, masks and frames.  Tool: tools/bench_flow_repair.py (each step a process under its own time "
        "limit).\nNothing is asserted; with synthetic weights nothing can be said about quality.  No kernel trace was taken.\n")


def main():
    ap = parser("flow_repair_bench.txt", STEPS)
    ap.add_argument("--parent", default="", help="a built checkout of the parent commit, for the headline step")
    args = ap.parse_args()
    if args.only:
        return run_only(args.only, lambda: run_step(args.only, args))
    return drive(__file__, HEAD, STEPS, args)


if __name__ == "__main__":
    sys.exit(main())
