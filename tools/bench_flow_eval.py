"""The optical-flow evaluation on the GPU: one JSON line with
  flow_metrics_ms_{sintel,n7_720p}   flow_metric_sums of one 436x1024 field read out of a 448x1024 stage-1-shaped tensor / of 7 fields
                                     at 720x1280, warm: median over `--windows` event-timed windows of `--iters` back-to-back calls, per
                                     call.  A window holds both launches and each call's host work (checks, two allocations from torch's
                                     caching allocator); the kernels' own time is what `rocprofv3 --kernel-trace --stats` reports for
                                     flow_epe_kernel / flow_epe_finish / flow_maxrad_kernel / flow_rgb_kernel when it runs this tool
  flow_to_rgb_ms_{sintel,n7_720p}    the same for flow_to_rgb
  *_onetouch_us                      the pass's one-touch bytes (metric: 16 B read per pixel; colour: 8 B read twice is still 8 B of
                                     HBM for fields that fit the cache, + 3 B written) over the 6.3 TB/s achievable HBM rate of VERDICT.md
  flow_loop_sps / full_loop_sps      Sintel-shaped samples per second of FlowEvaluator (FullModel.estimate_flow, metrics="host" and
                                     "device") against the same loop with the full model(pair, t, inference_mode=True) whose stage 2 is
                                     discarded - what the reference's script does: median and (min, max) over `--runs` runs each, run
                                     alternately in one process
Usage: python tools/bench_flow_eval.py [--iters 50] [--windows 7] [--runs 5] [--samples 8] [--skip-loops]"""
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
from ssm_amd.flow_eval import FlowEvaluator, clip_flow_samples, compute_metrics_host, flow_metric_sums, flow_to_rgb  # noqa: E402
from ssm_amd.weights import synthetic_frames_u8, synthetic_state_dict  # noqa: E402

HBM_BYTES_PER_S = 6.3e12


def call_ms(fn, iters, windows):
    for _ in range(5):
        fn()
    out = []
    for _ in range(windows):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(iters):
            fn()
        end.record()
        torch.cuda.synchronize()
        out.append(start.elapsed_time(end) / iters)
    return float(np.median(out))


def kernel_figures(dev, iters, windows):
    res = {}
    for tag, n, hp, wp, h, w, top in (("sintel", 1, 448, 1024, 436, 1024, 6), ("n7_720p", 7, 736, 1280, 720, 1280, 8)):
        g = torch.Generator(device="cpu").manual_seed(1)
        flow4 = (torch.randn(n, 4, hp, wp, generator=g) * 4).to(dev)
        gt = (torch.randn(n, h, w, 2, generator=g) * 4).to(dev)
        px = n * h * w
        res["flow_metrics_ms_" + tag] = round(call_ms(lambda: flow_metric_sums(flow4[:, 0:2], gt, top, 0, 0), iters, windows), 4)
        res["flow_metrics_onetouch_us_" + tag] = round(16.0 * px / HBM_BYTES_PER_S * 1e6, 2)
        res["flow_to_rgb_ms_" + tag] = round(call_ms(lambda: flow_to_rgb(flow4[:, 0:2], h, w, top, 0), iters, windows), 4)
        res["flow_to_rgb_onetouch_us_" + tag] = round(11.0 * px / HBM_BYTES_PER_S * 1e6, 2)
    return res


def full_forward_loop(model, samples, top, h):
    """The reference's loop (scripts/evaluate_optical_flow_results.py:47-69): full model, keep intermediate_outputs[0], host metrics."""
    epe = []
    for images, gt in samples:
        t = torch.full((1, 1, 1, 1, 1), 0.5, device=images.device)
        _, inter = model(images, t, iteration=None, inference_mode=True)
        flow01 = inter[0].permute(0, 2, 3, 1)[:, top:top + h].cpu().numpy()
        epe.append(compute_metrics_host(flow01, gt.cpu().numpy())[0])
    return epe


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0), out


def loop_figures(dev, runs, n_samples):
    cfg = load_config("superslomo_original.ini", synthetic_weight_overrides())
    model = FullModel(cfg)
    model.stage1_model.load_state_dict(synthetic_state_dict(1))
    model.stage2_model.load_state_dict(synthetic_state_dict(2))
    model = model.to(dev).eval()
    h, w = 436, 1024
    clip = synthetic_frames_u8(n_samples + 1, h, w, seed=42).permute(0, 2, 3, 1).contiguous().to(dev)
    g = torch.Generator(device="cpu").manual_seed(2)
    flows = torch.randn(n_samples, h, w, 2, generator=g) * 4                    # host ground truth, as a loader yields it
    samples = list(clip_flow_samples(clip, flows, cfg))

    def flow_loop(mode):
        ev = FlowEvaluator(cfg, model, h, w, metrics=mode)
        ev.run_evaluation(samples)
        return ev.EPE

    loops = {"flow_loop_host": lambda: flow_loop("host"), "flow_loop_device": lambda: flow_loop("device"),
             "full_loop": lambda: full_forward_loop(model, samples, 6, h)}
    sps = {k: [] for k in loops}
    epe = {}
    for k, fn in loops.items():          # warm-up: plans, code objects
        fn()
    for _ in range(runs):                # alternate, so drift of the box hits all three alike
        for k, fn in loops.items():
            s, epe[k] = timed(fn, n_samples)
            sps[k].append(s)
    assert epe["flow_loop_host"] == epe["full_loop"], "estimate_flow and the full forward's stage 1 must give the same EPE"
    res = {}
    for k, v in sps.items():
        res[k + "_sps"] = {"median": round(float(np.median(v)), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
    for k in ("flow_loop_host", "flow_loop_device"):
        res[k + "_over_full"] = round(res[k + "_sps"]["median"] / res["full_loop_sps"]["median"], 3)
        res[k + "_over_full_worst"] = round(res[k + "_sps"]["min"] / res["full_loop_sps"]["max"], 3)
    res["samples"] = n_samples
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--skip-loops", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_flow_eval needs the MI355X"
    dev = torch.device("cuda:0")
    res = kernel_figures(dev, a.iters, a.windows)
    if not a.skip_loops:
        res.update(loop_figures(dev, a.runs, a.samples))
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
