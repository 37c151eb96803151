"""Repair of repeated frames of the streamed video path (ssm_amd/video.py) on synthetic frames, in the manner of
tools/bench_detelecine.py: three steps, each a child process under its own `timeout`, chained - the first one that fails (or runs into
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
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "superslomo-videointerpolation-pytorch_amd")
for p in (ROOT, PKG, os.path.join(PKG, "scripts"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

from bench_fields import COPY_CEILING_BYTES_PER_S, alternated_ms  # noqa: E402

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
    import torch
    from models.superslomo_r import FullModel
    from ssm_amd import frames as F
    from ssm_amd import video as V
    from ssm_amd.config import load_config, synthetic_weight_overrides
    from ssm_amd.weights import synthetic_frames_u8, synthetic_state_dict
    cfg = load_config("superslomo_original.ini", synthetic_weight_overrides())
    model = FullModel(cfg)
    model.stage1_model.load_state_dict(synthetic_state_dict(1))
    model.stage2_model.load_state_dict(synthetic_state_dict(2))
    model = model.to(dev).eval()
    rgb = synthetic_frames_u8(BASE_FRAMES, H, W, seed=42).permute(0, 2, 3, 1).contiguous()
    matrix, crange, siting = V.default_matrix(H), V.LIMITED, V.CENTRED
    base = torch.cat([V.frames_to_yuv(F.frames_from_u8(rgb[i:i + 8].to(dev), cfg, True), H, W, siting, matrix, crange, cfg).cpu()
                      for i in range(0, BASE_FRAMES, 8)]).numpy()
    times = [2 + i % 2 for i in range(BASE_FRAMES)]          # 2, 3, 2, 3, ...
    repeated = np.repeat(base, times, axis=0)
    assert len(repeated) == 65
    acts, rep = V.dedup_host(repeated, H, W, siting)
    assert [r[1:3] for r in rep.log] == [(t - 1, True) for t in times[:-1]] + [(times[-1] - 1, False)], "the base clip moves: only the copies repeat"
    legs = ("dedup_upsample_rate_1_65_frames_720p", "upsample_rate_2_26_base_frames_720p")
    vis = dict(zip(legs, (V.VideoInterpolator(model, cfg, upsample_rate=1, n_streams=2, pairs_per_batch=1, matrix=matrix, dedup=True),
                          V.VideoInterpolator(model, cfg, upsample_rate=2, n_streams=2, pairs_per_batch=1, matrix=matrix))))
    secs, count = {k: [] for k in legs}, {}
    with tempfile.TemporaryDirectory(prefix="bench_dedup_") as tmp:
        paths = dict(zip(legs, (os.path.join(tmp, "repeated.y4m"), os.path.join(tmp, "base.y4m"))))
        for name, clip in zip(legs, (repeated, base)):
            with V.Y4MWriter(paths[name], W, H, rate=(60, 1), aspect=(1, 1), chroma="420jpeg") as wr:
                for p in clip:
                    wr.write_frame(p)
        for turn in range(runs + 1):          # turn 0: plans, pinned buffers' first touch
            for name in legs:
                t0 = time.perf_counter()
                with V.Y4MReader(paths[name]) as r:
                    with V.Y4MWriter.like(os.devnull, r) as w:
                        count[name] = vis[name].run(r, w)
                        w.f.flush()
                dt = time.perf_counter() - t0
                if turn > 0:
                    secs[name].append(dt)
    runs_log = vis[legs[0]].repeats
    assert count == {legs[0]: 65, legs[1]: 2 * BASE_FRAMES - 1} and len(runs_log) == BASE_FRAMES and sum(1 for r in runs_log if r[2]) == 25
    synthesised = {legs[0]: sum(t for t in times[:-1]) - 25, legs[1]: BASE_FRAMES - 1}

    def per_s(c, ts):
        v = [c / t for t in ts]
        return {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=[s for s, _ in STEPS], default=None, help="run this step in this process (what the driver starts)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dedup_bench.txt"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()
    if args.only:
        print(json.dumps({args.only: run_step(args.only, args)}))
        return 0
    head = ("Repair of repeated frames of the streamed video path (ssm_block_sad_fwd, RepeatSource, --dedup; DESIGN 3.12).\nOne MI355X, the "
            "default precision, synthetic weights and frames.  Tool: tools/bench_dedup.py (each step a process under its own time "
            "limit).\nNothing is asserted; with synthetic weights nothing can be said about quality.\n")
    with open(args.out, "w") as f:
        f.write(head)
    for step, limit in STEPS:
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--only", step, "--iters", str(args.iters),
               "--windows", str(args.windows), "--runs", str(args.runs)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        line = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else ""
        with open(args.out, "a") as f:
            f.write("\n== %s: `python tools/bench_dedup.py --only %s` (limit %d s, exit status %d) ==\n" % (step, step, limit, r.returncode))
            if r.returncode == 0:
                f.write(json.dumps(json.loads(line), indent=1) + "\n")
        print("%s: exit status %d %s" % (step, r.returncode, line), flush=True)
        if r.returncode != 0:          # a failure, a fault or a time limit: nothing more is started on the GPU
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
