"""The evaluator's metrics on the GPU against the host: one JSON line with
  frame_metric_sums_ms_n7_720p
                             frame_metric_sums of 7 frame pairs at 720x1280, warm: device events around `--iters` back-to-back
                             calls, per call.  The window holds both launches and each call's host work (checks, two allocations from
                             torch's caching allocator); the kernels' own time is what `rocprofv3 --kernel-trace` reports
  host_ms_per_frame_720p     eval_single_image (numpy PSNR / IE, scipy SSIM) of one 720p pair, wall clock
  evaluator_fps_host         Evaluator.run_evaluation frames/s, metrics="host", synthetic 720p clip of 17 images (2 windows, 14 frames)
  evaluator_fps_device       the same with metrics="device"
plus the largest differences of the two Evaluators' mean PSNR / SSIM / IE (what the host computes stays the yardstick).
Usage: python tools/bench_eval_metrics.py [--iters 50] [--host-frames 3] [--device-runs 5]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "superslomo-videointerpolation-pytorch_amd")
for p in (ROOT, PKG, os.path.join(PKG, "scripts")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from models.superslomo_r import FullModel  # noqa: E402
from ssm_amd.config import load_config, synthetic_weight_overrides  # noqa: E402
from ssm_amd.evaluation import Evaluator, clip_samples, eval_single_image, frame_metric_sums  # noqa: E402
from ssm_amd.weights import synthetic_frames_u8, synthetic_state_dict  # noqa: E402

H, W = 720, 1280


def sums_call_ms(clip, iters):
    t, o = clip[:7].contiguous(), clip[1:8].contiguous()
    for _ in range(5):
        frame_metric_sums(t, o)
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        frame_metric_sums(t, o)
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / iters


def host_ms_per_frame(clip_np, n):
    eval_single_image(clip_np[0], clip_np[1])
    t0 = time.perf_counter()
    for k in range(n):
        eval_single_image(clip_np[k], clip_np[k + 1])
    return (time.perf_counter() - t0) * 1e3 / n


def evaluator_run(cfg, model, clip, mode):
    ev = Evaluator(cfg, model, H, W, dataset="ADOBE", metrics=mode)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = ev.run_evaluation(clip_samples(clip, cfg, n_frames=2))
    torch.cuda.synchronize()
    return res, res["frames"] / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--host-frames", type=int, default=3)
    ap.add_argument("--device-runs", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_eval_metrics needs the MI355X"
    dev = torch.device("cuda:0")
    cfg = load_config("superslomo_original.ini", synthetic_weight_overrides())
    model = FullModel(cfg)
    model.stage1_model.load_state_dict(synthetic_state_dict(1))
    model.stage2_model.load_state_dict(synthetic_state_dict(2))
    model = model.to(dev).eval()
    clip_cpu = synthetic_frames_u8(17, H, W, seed=42).permute(0, 2, 3, 1).contiguous()
    clip = clip_cpu.to(dev)

    k_ms = sums_call_ms(clip, a.iters)
    h_ms = host_ms_per_frame(clip_cpu.numpy(), a.host_frames)
    evaluator_run(cfg, model, clip, "device")                                  # warm-up: model plans, code objects
    dev_runs = [evaluator_run(cfg, model, clip, "device") for _ in range(a.device_runs)]
    host_res, host_fps = evaluator_run(cfg, model, clip, "host")
    dev_res = dev_runs[-1][0]
    assert host_res["frames"] == dev_res["frames"] == 14, (host_res, dev_res)
    dev_fps = float(np.median([f for _, f in dev_runs]))
    print(json.dumps({
        "frame_metric_sums_ms_n7_720p": round(k_ms, 4),
        "host_ms_per_frame_720p": round(h_ms, 2),
        "evaluator_fps_host": round(host_fps, 3),
        "evaluator_fps_device": round(dev_fps, 2),
        "evaluator_speedup": round(dev_fps / host_fps, 1),
        "evaluator_frames": dev_res["frames"],
        "mean_diff": {k: abs(dev_res[k] - host_res[k]) for k in ("PSNR", "SSIM", "IE")},
    }))
    return 0


if __name__ == "__main__":
    sys.exit(main())
