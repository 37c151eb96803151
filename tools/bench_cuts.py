"""The scene cuts of the streamed video path (VideoInterpolator(scene_cut=)) on synthetic frames.  Two steps, each a child
process under its own `timeout`, chained: the first one that fails (or runs into its limit) ends the run.  Each step prints one JSON line:
  kernel   event-timed ssm_luma_sad_fwd (its memset included) on 7 frame pairs at 720p - frames n and n + 1 of 8 payloads in one buffer, as
           the streamed loop lays them out - beside device-to-device copies in the same run: one that reads all the bytes the kernel reads
           (and writes as many), one whose read and written bytes together are the kernel's bytes; median over `--windows` windows of
           `--iters` back-to-back calls, per call
  fps      output frames per second of wall time of VideoInterpolator.run, file to /dev/null, on a 720p clip at upsample_rate 8, in turns:
           without scene_cut and with it; 2 streams x 1 pair, both legs on the same two HIP streams (DESIGN 3.12 on why)
Nothing is asserted on the numbers.  Expectations they are there to test: the kernel sits near the copy's time for its bytes (the
accumulate kernel's 1.025 x and the tile stitch kernel's 1.16 x are the comparable figures in the project), and the stream rate with the
option lies inside the tool's own run-to-run spread (2 B per pixel read beside about 7 ms of work per pair).
Usage: python tools/bench_cuts.py [--out profiles/scene_cut_bench.txt] [--only kernel|fps] [--iters 20] [--windows 7] [--runs 3] [--frames 41]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time
from fractions import Fraction

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "superslomo-videointerpolation-pytorch_amd")
for p in (ROOT, PKG, os.path.join(PKG, "scripts"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
from bench_shutter import call_ms  # noqa: E402


STEPS = (("kernel", 180), ("fps", 600))          # step, its time limit in seconds
H, W = 720, 1280
THRESHOLD = Fraction(1, 10)          # a value for the run, not a recommendation: the synthetic clip moves steadily and holds no cut


def bench_kernel(dev, iters, windows):
    import numpy as np
    import torch
    from ssm_amd import video as V
    n = 7
    fb = V.frame_bytes(H, W, V.CENTRED)
    gen = torch.Generator(device="cpu").manual_seed(1)
    host = torch.randint(0, 256, (n + 1, fb), generator=gen, dtype=torch.uint8)
    buf = host.to(dev)
    sums = torch.empty(n, dtype=torch.int64, device=dev)
    nbytes = 2 * n * H * W          # what the kernel reads
    V.luma_sad(buf[:-1], buf[1:], H, W, out=sums)
    y = host.numpy()[:, :H * W].reshape(n + 1, H, W)
    assert sums.cpu().numpy().view(np.uint64).tolist() == V.luma_sad_host(y[:-1], y[1:]).tolist()
    src, dst = torch.empty(nbytes, dtype=torch.uint8, device=dev).random_(), torch.empty(nbytes, dtype=torch.uint8, device=dev)
    ms = call_ms(lambda: V.luma_sad(buf[:-1], buf[1:], H, W, out=sums), iters, windows)
    copy_all_ms = call_ms(lambda: dst.copy_(src), iters, windows)
    copy_half_ms = call_ms(lambda: dst[:nbytes // 2].copy_(src[:nbytes // 2]), iters, windows)
    return {"pairs": n, "plane": [H, W], "frame_bytes": fb, "bytes_read": nbytes, "ssm_luma_sad_fwd_ms": round(ms, 4),
            "d2d_copy_reading_the_same_bytes_ms": round(copy_all_ms, 4), "d2d_copy_read_plus_written_the_same_bytes_ms": round(copy_half_ms, 4),
            "sad_over_copy_reading_the_same_bytes": round(ms / copy_all_ms, 3),
            "sad_over_copy_read_plus_written_the_same_bytes": round(ms / copy_half_ms, 3), "sad_GB_per_s": round(nbytes / ms / 1e6, 1)}


def bench_fps(dev, runs, n_frames):
    import torch
    from models.superslomo_r import FullModel
    from ssm_amd import frames as F
    from ssm_amd import video as V
    from ssm_amd.config import load_config, synthetic_weight_overrides
    from ssm_amd.weights import synthetic_frames_u8, synthetic_state_dict
    assert 2 <= n_frames <= 43, "synthetic_frames_u8 holds 43 frames of this size at the most"
    cfg = load_config("superslomo_original.ini", synthetic_weight_overrides())
    model = FullModel(cfg)
    model.stage1_model.load_state_dict(synthetic_state_dict(1))
    model.stage2_model.load_state_dict(synthetic_state_dict(2))
    model = model.to(dev).eval()
    rgb = synthetic_frames_u8(n_frames, H, W, seed=42).permute(0, 2, 3, 1).contiguous()
    matrix, crange, siting = V.default_matrix(H), V.LIMITED, V.CENTRED
    payloads = torch.cat([V.frames_to_yuv(F.frames_from_u8(rgb[i:i + 8].to(dev), cfg, True), H, W, siting, matrix, crange, cfg).cpu()
                          for i in range(0, n_frames, 8)]).numpy()
    legs = {"no_scene_cut": V.VideoInterpolator(model, cfg, upsample_rate=8, n_streams=2, pairs_per_batch=1),
            "scene_cut": V.VideoInterpolator(model, cfg, upsample_rate=8, n_streams=2, pairs_per_batch=1, scene_cut=THRESHOLD)}
    fps, frames_written = {name: [] for name in legs}, {}
    with tempfile.TemporaryDirectory(prefix="bench_cuts_") as tmp:
        src = os.path.join(tmp, "clip.y4m")
        with V.Y4MWriter(src, W, H, rate=(30, 1), aspect=(1, 1), chroma="420jpeg") as wr:
            for p in payloads:
                wr.write_frame(p)
        for turn in range(runs + 2):          # turn 0: plans, pinned buffers' first touch; turn 1: the first run on the shared streams
            if turn == 1:
                pipes = [vi._pipe[1] for vi in legs.values()]
                pipes[1].streams = pipes[0].streams
            for name, vi in legs.items():
                with V.Y4MReader(src) as r, V.Y4MWriter.like(os.devnull, r, rate=(240, 1)) as w:
                    t0 = time.perf_counter()
                    k = vi.run(r, w)
                    w.f.flush()
                    dt = time.perf_counter() - t0
                frames_written[name] = k
                if turn > 1:
                    fps[name].append(k / dt)
    rec = {name: {"output_frames_per_s": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2),
                  "frames_written": frames_written[name]} for name, v in fps.items()}
    rec["scene_cut"]["cuts"] = [[i, float(s)] for i, s in legs["scene_cut"].cuts]
    rec["scene_cut_over_no_scene_cut_time_per_output_frame"] = round(rec["no_scene_cut"]["output_frames_per_s"] /
                                                                     rec["scene_cut"]["output_frames_per_s"], 4)
    rec["note"] = ("%d frames of %dx%d, upsample_rate 8, file to /dev/null, 2 streams x 1 pair, legs in turns on the same two HIP streams, %d timed "
                   "runs each; threshold %s" % (n_frames, W, H, runs, THRESHOLD))
    return rec


def run_step(step, args):
    import torch
    assert torch.cuda.is_available(), "bench_cuts.py measures on the GPU; there is no CPU path"
    dev = torch.device("cuda:0")
    return bench_kernel(dev, args.iters, args.windows) if step == "kernel" else bench_fps(dev, args.runs, args.frames)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=[s for s, _ in STEPS], default=None, help="run this step in this process (what the driver starts)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_cut_bench.txt"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--frames", type=int, default=41)
    args = ap.parse_args()
    if args.only:
        print(json.dumps({args.only: run_step(args.only, args)}))
        return 0
    head = ("Scene cuts of the streamed video path (luma differences summed on the GPU, the decision on the writer thread; DESIGN 3.12).\n"
            "One MI355X, the default precision, synthetic weights and frames.  Tool: tools/bench_cuts.py (each step a process under its own "
            "time limit).\nExpected: the kernel near a copy's time for its bytes (accumulate kernel 1.025 x, tile stitch kernel 1.16 x); the "
            "stream rate with the option inside the run-to-run spread.  Nothing is asserted.\n")
    with open(args.out, "w") as f:
        f.write(head)
    for step, limit in STEPS:
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--only", step, "--iters", str(args.iters),
               "--windows", str(args.windows), "--runs", str(args.runs), "--frames", str(args.frames)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        line = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else ""
        with open(args.out, "a") as f:
            f.write("\n== %s: `python tools/bench_cuts.py --only %s` (limit %d s, exit status %d) ==\n" % (step, step, limit, r.returncode))
            if r.returncode == 0:
                f.write(json.dumps(json.loads(line), indent=1) + "\n")
        print("%s: exit status %d %s" % (step, r.returncode, line), flush=True)
        if r.returncode != 0:          # a failure, a fault or a time limit: nothing more is started on the GPU
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
