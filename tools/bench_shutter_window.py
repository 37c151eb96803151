"""The shutter windows (VideoInterpolator(shutter_window=)) on synthetic frames, in the manner of tools/bench_shutter_light.py.
Two steps, each a child process under its own `timeout`, chained: the first one that fails (or runs into its limit) ends the run.  Each
step prints one JSON line:
  kernel   event-timed weighted accumulate kernels on 8 frames at 736x1280 (init = 1, the triangle's weights and scale: 8 planes read, one
           written) - coded, srgb, pq and hlg (the three lights with encode = 1) - each beside its unweighted sibling on the same frames
           and a device-to-device copy of the same bytes (read + written).  The three are ALTERNATED: every one of `--windows` windows
           times `--iters` back-to-back calls of the copy, then of the sibling, then of the weighted kernel; the figures are the medians
           over the windows, per call, with the windows' min and max as the run's own spread
  fps      output frames per second of wall time of VideoInterpolator.run, file to /dev/null, on a 720p clip at 60:1 converted to 24:1
           (step 5/2) with shutter 180 degrees in 8 samples, in turns: shutter_window "box" and "triangle"; 2 streams x 1 pair, both legs
           on the same two HIP streams
Nothing is asserted on the numbers.  Expectations they are there to test: the coded weighted kernel stays at the copy's time like its
sibling (it is read-bound and the weights are scalar operands), and the stream rate stays inside its run-to-run spread, since stage 2
dominates.
Usage: python tools/bench_shutter_window.py [--out profiles/shutter_window_bench.txt] [--only kernel|fps] [--iters 20] [--windows 7]
       [--runs 3] [--frames 41]"""
import argparse
import ctypes
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

from bench_shutter import COPY_CEILING_BYTES_PER_S, H, SAMPLES, SHUTTER, W  # noqa: E402

STEPS = (("kernel", 240), ("fps", 600))          # step, its time limit in seconds
WINDOW = "triangle"


def alternated_ms(fns, iters, windows):
    """{name: (median, min, max) ms per call}: every window times `iters` back-to-back calls of each function in turn."""
    import torch
    for fn in fns.values():
        for _ in range(5):
            fn()
    out = {name: [] for name in fns}
    for _ in range(windows):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out[name].append(e0.elapsed_time(e1) / iters)
    return {name: (statistics.median(v), min(v), max(v)) for name, v in out.items()}


def bench_kernel(dev, iters, windows):
    import torch
    from ssm_amd import hipbind as hb
    from ssm_amd import video as V
    from ssm_amd.frames import cfg_mean_std
    n, hp, wp = 8, 736, 1280
    mean, std = cfg_mean_std(None)
    m, s = (torch.tensor(x).view(1, 3, 1, 1) for x in (mean, std))
    gen = torch.Generator(device="cpu").manual_seed(1)
    frames = (((torch.rand((n, 3, hp, wp), generator=gen) * 1.1 - 0.05) - m) / s).to(dev)          # coded values in [-0.05, 1.05]
    acc = torch.empty(1, 3, hp, wp, device=dev)
    nbytes = 4 * 3 * hp * wp * (n + 1)          # 8 planes read, one written
    src, dst = torch.randn(nbytes // 8, device=dev), torch.empty(nbytes // 8, device=dev)          # read nbytes / 2, write nbytes / 2
    w, scale = V.shutter_window(WINDOW, n)
    wts, scale = (ctypes.c_float * n)(*[float(x) for x in w]), float(scale)          # as the binding takes them: built once
    floats = lambda x: (ctypes.c_float * len(x))(*[float(y) for y in x])
    nm = (floats(mean), floats(std))
    kind_pq, row_pq = V.hdr_light("pq")
    kind_hlg, row_hlg = V.hdr_light("hlg")
    srgb, pq, hlg = floats(V.light_curve("srgb")), floats(row_pq), floats(row_hlg)
    pairs = {"coded": (lambda: hb.frames_accumulate(frames, acc, 1, 0.125),
                       lambda: hb.frames_accumulate(frames, acc, 1, scale, weights=wts)),
             "srgb": (lambda: hb.frames_accumulate_light(frames, acc, 1, 0.125, *nm, srgb, 1),
                      lambda: hb.frames_accumulate_light(frames, acc, 1, scale, *nm, srgb, 1, weights=wts)),
             "pq": (lambda: hb.frames_accumulate_hdr(frames, acc, 1, 0.125, *nm, kind_pq, pq, 1),
                    lambda: hb.frames_accumulate_hdr(frames, acc, 1, scale, *nm, kind_pq, pq, 1, weights=wts)),
             "hlg": (lambda: hb.frames_accumulate_hdr(frames, acc, 1, 0.125, *nm, kind_hlg, hlg, 1),
                     lambda: hb.frames_accumulate_hdr(frames, acc, 1, scale, *nm, kind_hlg, hlg, 1, weights=wts))}
    rec = {"frames": n, "canvas": [hp, wp], "init": 1, "window": WINDOW, "weights": [float(x) for x in w], "scale": scale,
           "bytes_read_and_written": nbytes, "ms_at_copy_ceiling": round(1e3 * nbytes / COPY_CEILING_BYTES_PER_S, 4),
           "iters_per_window": iters, "windows": windows}
    for name, (plain, weighted) in pairs.items():
        t = alternated_ms({"copy": lambda: dst.copy_(src), "unweighted": plain, "weighted": weighted}, iters, windows)
        rec[name] = {k: {"ms": round(v[0], 4), "min": round(v[1], 4), "max": round(v[2], 4)} for k, v in t.items()}
        rec[name]["weighted_over_unweighted"] = round(t["weighted"][0] / t["unweighted"][0], 3)
        rec[name]["weighted_over_copy"] = round(t["weighted"][0] / t["copy"][0], 3)
        rec[name]["unweighted_over_copy"] = round(t["unweighted"][0] / t["copy"][0], 3)
    return rec


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
    legs = {window: V.VideoInterpolator(model, cfg, n_streams=2, pairs_per_batch=1, target_rate=(24, 1), shutter=SHUTTER, shutter_samples=SAMPLES,
                                        shutter_window=window) for window in ("box", WINDOW)}
    fps, frames_written = {name: [] for name in legs}, {}
    with tempfile.TemporaryDirectory(prefix="bench_shutter_window_") as tmp:
        src = os.path.join(tmp, "clip.y4m")
        with V.Y4MWriter(src, W, H, rate=(60, 1), aspect=(1, 1), chroma="420jpeg") as wr:
            for p in payloads:
                wr.write_frame(p)
        for turn in range(runs + 2):          # turn 0: plans, pinned buffers' first touch; turn 1: the first run on the shared streams
            if turn == 1:
                pipes = [vi._pipe[1] for vi in legs.values()]
                pipes[1].streams = pipes[0].streams
            for name, vi in legs.items():
                with V.Y4MReader(src) as r, V.Y4MWriter.like(os.devnull, r, rate=(24, 1)) as w:
                    t0 = time.perf_counter()
                    k = vi.run(r, w)
                    w.f.flush()
                    dt = time.perf_counter() - t0
                frames_written[name] = k
                if turn > 1:
                    fps[name].append(k / dt)
    rec = {name: {"output_frames_per_s": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2),
                  "frames_written": frames_written[name]} for name, v in fps.items()}
    rec["%s_over_box_time_per_output_frame" % WINDOW] = round(rec["box"]["output_frames_per_s"] / rec[WINDOW]["output_frames_per_s"], 3)
    rec["note"] = ("%d frames of %dx%d at 60:1 -> 24:1 (step 5/2), shutter 180 degrees in %d samples, file to /dev/null, 2 streams x 1 pair, legs "
                   "in turns on the same two HIP streams, %d timed runs each" % (n_frames, W, H, SAMPLES, runs))
    return rec


def run_step(step, args):
    import torch
    assert torch.cuda.is_available(), "bench_shutter_window.py measures on the GPU; there is no CPU path"
    dev = torch.device("cuda:0")
    return bench_kernel(dev, args.iters, args.windows) if step == "kernel" else bench_fps(dev, args.runs, args.frames)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=[s for s, _ in STEPS], default=None, help="run this step in this process (what the driver starts)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shutter_window_bench.txt"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--frames", type=int, default=41)
    args = ap.parse_args()
    if args.only:
        print(json.dumps({args.only: run_step(args.only, args)}))
        return 0
    head = ("Shutter windows of the streamed video path (weighted sums of the sub-frames on the GPU; DESIGN 3.12).\n"
            "One MI355X, the default precision, synthetic weights and frames.  Tool: tools/bench_shutter_window.py (each step a process under its "
            "own time limit;\nthe copy, the unweighted kernel and the weighted kernel alternate window by window in one run).\nExpected: the coded "
            "weighted kernel at the copy's time, like its sibling; the stream rate inside its run-to-run spread, since stage 2 dominates.\n"
            "Nothing is asserted.\n")
    with open(args.out, "w") as f:
        f.write(head)
    for step, limit in STEPS:
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--only", step, "--iters", str(args.iters),
               "--windows", str(args.windows), "--runs", str(args.runs), "--frames", str(args.frames)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        line = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else ""
        with open(args.out, "a") as f:
            f.write("\n== %s: `python tools/bench_shutter_window.py --only %s` (limit %d s, exit status %d) ==\n" % (step, step, limit, r.returncode))
            if r.returncode == 0:
                f.write(json.dumps(json.loads(line), indent=1) + "\n")
        print("%s: exit status %d %s" % (step, r.returncode, line), flush=True)
        if r.returncode != 0:          # a failure, a fault or a time limit: nothing more is started on the GPU
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
