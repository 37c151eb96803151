"""Blocks that do not change of the streamed video path (ssm_amd/video.py) on synthetic frames, in the manner of
tools/bench_dedup.py: three steps, each a child process under its own `timeout`, chained - the first one that fails (or runs into its
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
    clip = keep_quarter(np.concatenate([base, base[-2::-1]]), siting, 8)          # there and back: 65 frames, neighbours always differ
    assert len(clip) == 65
    _, per_pair = V.static_paste_host(np.zeros((64, 1, clip.shape[1]), np.uint8), clip[:-1], clip[1:], H, W, siting, 8, 0)
    legs = ("static_0_upsample_rate_8_65_frames_720p", "upsample_rate_8_65_frames_720p")
    vis = dict(zip(legs, (V.VideoInterpolator(model, cfg, upsample_rate=8, n_streams=2, pairs_per_batch=1, matrix=matrix, static=0),
                          V.VideoInterpolator(model, cfg, upsample_rate=8, n_streams=2, pairs_per_batch=1, matrix=matrix))))
    secs, count = {k: [] for k in legs}, {}
    with tempfile.TemporaryDirectory(prefix="bench_static_") as tmp:
        path = os.path.join(tmp, "clip.y4m")
        with V.Y4MWriter(path, W, H, rate=(30, 1), aspect=(1, 1), chroma="420jpeg") as wr:
            for p in clip:
                wr.write_frame(p)
        for turn in range(runs + 1):          # turn 0: plans, pinned buffers' first touch
            for name in legs:
                t0 = time.perf_counter()
                with V.Y4MReader(path) as r:
                    with V.Y4MWriter.like(os.devnull, r) as w:
                        count[name] = vis[name].run(r, w)
                        w.f.flush()
                dt = time.perf_counter() - t0
                if turn > 0:
                    secs[name].append(dt)
    kept = vis[legs[0]].static
    assert count == {k: 64 * 8 + 1 for k in legs} and [s for _, s, _ in kept] == per_pair.tolist() and vis[legs[1]].static == []

    def per_s(c, ts):
        v = [c / t for t in ts]
        return {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=[s for s, _ in STEPS], default=None, help="run this step in this process (what the driver starts)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "static_bench.txt"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()
    if args.only:
        print(json.dumps({args.only: run_step(args.only, args)}))
        return 0
    head = ("Blocks that do not change of the streamed video path (ssm_static_paste_fwd, --static; DESIGN 3.12).\nOne MI355X, the default "
            "precision, synthetic weights and frames.  Tool: tools/bench_static.py (each step a process under its own time limit).\n"
            "Nothing is asserted; with synthetic weights nothing can be said about quality.\n")
    with open(args.out, "w") as f:
        f.write(head)
    for step, limit in STEPS:
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--only", step, "--iters", str(args.iters),
               "--windows", str(args.windows), "--runs", str(args.runs)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        line = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else ""
        with open(args.out, "a") as f:
            f.write("\n== %s: `python tools/bench_static.py --only %s` (limit %d s, exit status %d) ==\n" % (step, step, limit, r.returncode))
            if r.returncode == 0:
                f.write(json.dumps(json.loads(line), indent=1) + "\n")
        print("%s: exit status %d %s" % (step, r.returncode, line), flush=True)
        if r.returncode != 0:          # a failure, a fault or a time limit: nothing more is started on the GPU
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
