"""The coarse-flow mode (flow_scale = 2 | 4: U-Nets at 1/s of the frame's size, synthesis at full size; an approximation of the
reference's output, not parity) on synthetic frames: one JSON line with
  kernels     event-timed calls of ssm_synthesize_upscaled_fwd (s = 2 and 4) beside ssm_synthesize_fwd at the same full size, one pair at 7
              interpolation times, at 2176x3840 and 768x1280: median over `--windows` windows of `--iters` back-to-back calls, per call; the
              one-touch bytes of the call (every tensor element read or written once: frames 24 B per pixel of the PAIR, maps and output
              per frame) and their fraction of the 6.29 TB/s copy ceiling; ns per output pixel.  Every kernel gathers at random
              displacements of up to +-4 full-size pixels per axis (the maps hold 4/s low-resolution pixels).  The kernels' own time is what
              `rocprofv3 --kernel-trace --stats` reports when it runs this tool with --only kernels
  fps         frames per second of PairPipeline.submit in f32w with flow_scale 1, 2 and 4 on one box: 2160p (3 streams x 1 pair) and 720p
              (3 streams x 2 pairs), 7 times per pair.  The three settings ALTERNATE, `--runs` runs each (a pipeline is built, warmed,
              timed and freed per run); flow_scale=1 of the same call is the comparison (it is the default path).  Reported: every
              run, the medians, the ratios median to median and whether the slowest coarse run beats the fastest full one
  closeness   PSNR (on denormalised RGB in [0,1]) of the mode's frames against the flow_scale=1 frames of the same pair, on the two
              synthetic frame families (texture, edges) at 768x1280.  With synthetic weights this says nothing about a trained model:
              reported, not asserted
Usage: python tools/bench_coarse.py [--only kernels|fps|closeness] [--iters 20] [--windows 7] [--runs 3] [--passes-4k 12] [--passes-720 48]"""
import argparse
import gc
import json
import statistics
import time

from video_bench import COPY_CEILING_BYTES_PER_S, call_ms          # and the import path

import torch  # noqa: E402

from ssm_amd import hipbind as hb  # noqa: E402
from ssm_amd.engine import PairPipeline  # noqa: E402
from ssm_amd.frames import padded_dims  # noqa: E402
from ssm_amd.weights import IMAGENET_MEAN, IMAGENET_STD, synthetic_frames, synthetic_state_dict  # noqa: E402

NT = 7
SCALES = (1, 2, 4)


def kernel_record(ms, nbytes, pixels):
    ideal_ms = 1e3 * nbytes / COPY_CEILING_BYTES_PER_S
    return {"ms": round(ms, 4), "one_touch_bytes": nbytes, "one_touch_ms": round(ideal_ms, 4), "fraction_of_copy_ceiling": round(ideal_ms / ms, 3),
            "ns_per_output_pixel": round(1e6 * ms / pixels, 4)}


def bench_kernels(dev, iters, windows):
    lib = hb.load()
    res = {}
    for H, W in ((2176, 3840), (768, 1280)):
        g = torch.Generator(device="cpu").manual_seed(H)
        img6 = torch.randn(1, 6, H, W, generator=g).to(dev)
        t = torch.linspace(0.125, 0.875, NT).to(dev)
        y3 = torch.empty(NT, 3, H, W, device=dev)
        i6 = hb.view_of(img6)
        i6.sb = 0
        px = NT * H * W
        rec = {}
        for s in (2, 4):
            aux = torch.empty(NT, 5, H // s, W // s, device=dev)
            aux[:, 0:4] = (torch.rand(NT, 4, H // s, W // s, generator=g).to(dev) * 2.0 - 1.0) * (4.0 / s)          # +-4 full-size pixels
            aux[:, 4] = 0.05 + 0.9 * torch.rand(NT, H // s, W // s, generator=g).to(dev)

            def up(aux=aux, s=s):
                hb.check(lib.ssm_synthesize_upscaled_fwd(i6, hb.view_of(aux), t.data_ptr(), hb.view_of(y3), NT, H, W, s, hb.stream_ptr()))
            nbytes = 12 * px + 24 * H * W + 20 * px // (s * s)
            rec["ssm_synthesize_upscaled_fwd_s%d" % s] = kernel_record(call_ms(up, iters, windows), nbytes, px)
            del aux
        # the default mode's synthesis at the same size and the same displacements (+-3 approximated, +-1 residual): reads channels 6..9 of its 16-channel argument (given here as a 4-channel tensor
        # behind a view whose origin lies 6 channels back, as the engine does in the split modes) and the 5-channel map
        est = (torch.rand(NT, 4, H, W, generator=g) * 6.0 - 3.0).to(dev)
        out5 = (torch.rand(NT, 5, H, W, generator=g) * 2.0 - 1.0).to(dev)
        ev = hb.view_of(est)
        in16 = hb.SsmView(ev.ptr - 4 * 6 * ev.sc, ev.sb, ev.sc, ev.sh)

        def full():
            hb.check(lib.ssm_synthesize_fwd(i6, in16, hb.view_of(out5), t.data_ptr(), hb.view_of(y3), hb.NULL_VIEW, NT, H, W, hb.stream_ptr()))
        rec["ssm_synthesize_fwd"] = kernel_record(call_ms(full, iters, windows), (12 + 16 + 20) * px + 24 * H * W, px)
        rec["note"] = "one pair, %d times, %dx%d; frames batch-broadcast (sb = 0)" % (NT, H, W)
        res["%dx%d" % (H, W)] = rec
        del est, out5, y3, img6
        torch.cuda.empty_cache()
    return res


def pairs_for(P, H, W, dev, family="texture", seed=42):
    x = synthetic_frames(P + 1, H, W, seed=seed, family=family)[0].to(dev)
    return torch.cat([x[:-1], x[1:]], 1).contiguous()


def bench_fps(dev, sd1, sd2, runs, passes_4k, passes_720):
    res = {}
    t = torch.linspace(0.125, 0.875, NT).to(dev)
    for name, h, w, P, passes in (("2160p", 2160, 3840, 1, passes_4k), ("720p", 720, 1280, 2, passes_720)):
        fps = {s: [] for s in SCALES}
        for _ in range(runs):          # one pipeline alive at a time: three 4K engines of the full-size mode take most of the device's memory
            for s in SCALES:
                (Hp, Wp), _ = padded_dims(h, w, 32 * s)
                pipe = PairPipeline(sd1, sd2, NT, Hp, Wp, dev, True, "f32w", n_streams=3, pairs_per_batch=P, flow_scale=s)
                img6 = pairs_for(P, Hp, Wp, dev)

                def run(n):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(n):
                        pipe.submit(img6, t)
                    pipe.sync()
                    torch.cuda.synchronize()
                    return n * P * NT / (time.perf_counter() - t0)

                run(6)          # plans, code objects, every slot of the pipeline
                fps[s].append(run(passes))
                del pipe, img6, run
                gc.collect()
                torch.cuda.empty_cache()
        med = {s: statistics.median(fps[s]) for s in SCALES}
        rec = {"flow_scale_%d" % s: {"canvas": list(padded_dims(h, w, 32 * s)[0]), "frames_per_s": [round(v, 2) for v in fps[s]],
                                     "median": round(med[s], 2)} for s in SCALES}
        for s in (2, 4):
            rec["flow_scale_%d" % s]["ratio_to_flow_scale_1_median_to_median"] = round(med[s] / med[1], 3)
            rec["flow_scale_%d" % s]["slowest_run_beats_fastest_full_run"] = min(fps[s]) > max(fps[1])
        rec["note"] = ("interpolated frames per second of wall time, PairPipeline f32w, 3 streams x %d pair(s), %d times, %d passes per run, "
                       "settings alternated; peak device memory %d MiB" % (P, NT, passes, torch.cuda.max_memory_allocated(dev) >> 20))
        res[name] = rec
    return res


def bench_closeness(dev, sd1, sd2):
    H, W = 768, 1280
    t = torch.linspace(0.125, 0.875, NT).to(dev)
    mean = torch.tensor(IMAGENET_MEAN, device=dev).view(1, 3, 1, 1)
    std = torch.tensor(IMAGENET_STD, device=dev).view(1, 3, 1, 1)
    rgb = lambda x: (x * std + mean).clamp(0, 1).double()      # noqa: E731
    res = {"size": [H, W], "note": "PSNR of flow_scale=s frames against flow_scale=1 frames of the same pair, denormalised RGB in [0,1], "
                                   "synthetic weights: no statement about a trained model"}
    for family in ("texture", "edges"):
        img6 = pairs_for(1, H, W, dev, family=family, seed=7)
        outs = {}
        for s in SCALES:
            pipe = PairPipeline(sd1, sd2, NT, H, W, dev, True, "f32w", n_streams=1, flow_scale=s)
            outs[s] = pipe.submit(img6, t, clone=True)
            pipe.sync()
            torch.cuda.synchronize()
            del pipe
        ref = rgb(outs[1])
        res[family] = {}
        for s in (2, 4):
            mse = ((rgb(outs[s]) - ref) ** 2).mean().item()
            res[family]["flow_scale_%d_psnr_db" % s] = round(10.0 * torch.log10(torch.tensor(1.0 / max(mse, 1e-30))).item(), 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("kernels", "fps", "closeness"), default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--passes-4k", type=int, default=12)
    ap.add_argument("--passes-720", type=int, default=48)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_coarse.py measures on the GPU; there is no CPU path"
    dev = torch.device("cuda:0")
    want = (args.only,) if args.only else ("kernels", "fps", "closeness")
    res = {"mode": "coarse flow: approximation of the reference's output, not parity; U-Nets at 1/s"}
    if "kernels" in want:
        res["kernels"] = bench_kernels(dev, args.iters, args.windows)
    if "fps" in want or "closeness" in want:
        sd1 = {k: v.to(dev) for k, v in synthetic_state_dict(1).items()}
        sd2 = {k: v.to(dev) for k, v in synthetic_state_dict(2).items()}
        if "fps" in want:
            res["fps"] = bench_fps(dev, sd1, sd2, args.runs, args.passes_4k, args.passes_720)
        if "closeness" in want:
            res["closeness"] = bench_closeness(dev, sd1, sd2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
