"""The streamed video path (ssm_amd.video, scripts/interpolate_video.py) on a synthetic 1280x720 clip: one JSON line with
  kernels            event-timed calls on 7 frames of ssm_frames_from_yuv_fwd / ssm_frames_to_yuv_fwd (4:2:0 centred, BT.709 limited)
                     beside ssm_frames_from_u8_fwd / ssm_frames_to_u8_fwd on the same frames: median over `--windows` windows of `--iters`
                     back-to-back calls, per call, the one-touch bytes of the call and their fraction of the 6.29 TB/s copy ceiling.
                     A window holds each call's host work too; the kernels' own time is what `rocprofv3 --kernel-trace --stats` reports
                     when it runs this tool
  video_fps          output frames per second of VideoInterpolator, file to file and file to /dev/null: wall time of run(), plans warm,
                     reading the clip included; median and (min, max) over `--runs` runs
  png_fps            the same clip as a folder of PNGs through scripts/visualize_interpolation.py (unchanged by the video path, so this
                     measures it as it was): wall time of main(), output frames / s
  timeline_fps       the arbitrary-rate path beside the fixed grid at the same times per pair: target_rate 75:1 on the 30:1 clip (step = 2/5,
                     the pattern of 24 -> 60, slots = 2) and upsample_rate = 3 (two times per pair as well), file to /dev/null, run in
                     turns in one process on the same two HIP streams; SYNTHESISED frames per second (frames passed through not counted), median and (min, max)
The clip (`--frames`, 41 by default: synthetic_frames_u8 moves its window 3 px per frame and has room for 43) is built from it, written below a temporary directory and deleted afterwards.
Usage: python tools/bench_video.py [--frames 41] [--iters 20] [--windows 7] [--runs 3] [--skip-e2e] [--skip-png] [--skip-timeline]
[--png-frames N]"""
import argparse
import json
import os
import shutil
import statistics
import tempfile
import time

from video_bench import (COPY_CEILING_BYTES_PER_S, call_ms, per_s, share_streams, synthetic_model, timed_legs,          # and the import path
                         write_y4m)

import torch  # noqa: E402

from ssm_amd import frames as F  # noqa: E402
from ssm_amd import video as V  # noqa: E402
from ssm_amd.weights import synthetic_frames_u8  # noqa: E402

H, W, RATE = 720, 1280, 8


def kernel_record(ms, nbytes):
    ideal_ms = 1e3 * nbytes / COPY_CEILING_BYTES_PER_S
    return {"ms": round(ms, 4), "one_touch_bytes": nbytes, "one_touch_ms": round(ideal_ms, 4), "fraction_of_copy_ceiling": round(ideal_ms / ms, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=41)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--skip-png", action="store_true")
    ap.add_argument("--skip-timeline", action="store_true")
    ap.add_argument("--png-frames", type=int, default=0, help="frames of the clip the PNG tool gets (0 = all)")
    args = ap.parse_args()
    assert 2 <= args.frames <= 43, "synthetic_frames_u8 holds 43 frames of this size at the most"
    dev = torch.device("cuda:0")
    model, cfg = synthetic_model(dev)

    # the payloads of video_bench.synthetic_payloads, made here because the kernels and the PNG leg below take the RGB frames too
    rgb = synthetic_frames_u8(args.frames, H, W, seed=42).permute(0, 2, 3, 1).contiguous()          # [n,H,W,3] uint8, host
    matrix, crange, siting = V.default_matrix(H), V.LIMITED, V.CENTRED
    payloads = torch.cat([V.frames_to_yuv(F.frames_from_u8(rgb[i:i + 8].to(dev), cfg, True), H, W, siting, matrix, crange, cfg).cpu()
                          for i in range(0, args.frames, 8)]).numpy()
    res = {"clip": {"frames": args.frames, "height": H, "width": W, "chroma": "420jpeg", "upsample_rate": RATE}}

    # ---- the four frame kernels on the same 7 frames ---------------------------------------------------------------------------------
    n = 7
    (hp, wp), _ = F.padded_dims(H, W)
    yuv7, rgb7 = torch.from_numpy(payloads[:n]).to(dev), rgb[:n].to(dev)
    x = F.frames_from_u8(rgb7, cfg, True)
    planes = torch.empty_like(x)
    codes = torch.empty(n, V.frame_bytes(H, W, siting), dtype=torch.uint8, device=dev)
    fp32_bytes = n * 3 * hp * wp * 4
    res["kernels"] = {
        "frames": n,
        "ssm_frames_from_yuv_fwd": kernel_record(call_ms(lambda: V.frames_from_yuv(yuv7, H, W, siting, matrix, crange, cfg, True, out=planes),
                                                         args.iters, args.windows), yuv7.numel() + fp32_bytes),
        "ssm_frames_from_u8_fwd": kernel_record(call_ms(lambda: F.frames_from_u8(rgb7, cfg, True), args.iters, args.windows),
                                                rgb7.numel() + fp32_bytes),
        "ssm_frames_to_yuv_fwd": kernel_record(call_ms(lambda: V.frames_to_yuv(x, H, W, siting, matrix, crange, cfg, out=codes),
                                                       args.iters, args.windows), codes.numel() + n * 3 * H * W * 4),
        "ssm_frames_to_u8_fwd": kernel_record(call_ms(lambda: F.frames_to_u8(x, H, W, cfg, saturate=True), args.iters, args.windows),
                                              rgb7.numel() + n * 3 * H * W * 4),
        "note": "per call on 7 frames of 720x1280 (canvas 736x1280); the RGB calls allocate their output, the video calls write into a given one",
    }
    del x, planes, codes, yuv7, rgb7

    tmp = tempfile.mkdtemp(prefix="bench_video_")
    try:
        src = os.path.join(tmp, "clip.y4m")
        write_y4m(src, payloads, W, H, (30, 1))
        if not args.skip_e2e:
            vi = V.VideoInterpolator(model, cfg, upsample_rate=RATE, n_streams=2, pairs_per_batch=1)

            def run(dst, frames_limit=None):
                with V.Y4MReader(src) as r, V.Y4MWriter.like(dst, r, rate=V.output_rate(r.rate, RATE)) as w:
                    t0 = time.perf_counter()
                    k = vi.run(r, w)
                    w.f.flush()
                    return k, time.perf_counter() - t0

            run(os.devnull)          # plans, pinned buffers' first touch
            rec = {}
            for name, dst in (("file_to_file", os.path.join(tmp, "out.y4m")), ("file_to_devnull", os.devnull)):
                fps = []
                for _ in range(args.runs):
                    k, dt = run(dst)
                    fps.append(k / dt)
                rec[name] = {"frames_per_s": round(statistics.median(fps), 2), "min": round(min(fps), 2), "max": round(max(fps), 2),
                             "frames_written": k}
            rec["note"] = ("output frames (originals included) per second of wall time of VideoInterpolator.run, 2 streams x 1 pair, the "
                           "precision mode of FullModel.interpolate; peak device memory %d MiB" % (torch.cuda.max_memory_allocated(dev) >> 20))
            res["video_fps"] = rec
        if not args.skip_timeline:
            legs = {"step_2_5_target_75": (V.VideoInterpolator(model, cfg, n_streams=2, pairs_per_batch=1, target_rate=(75, 1)), (75, 1)),
                    "upsample_rate_3": (V.VideoInterpolator(model, cfg, upsample_rate=3, n_streams=2, pairs_per_batch=1), (90, 1))}
            synth = {"step_2_5_target_75": sum(1 for _, t in V.Timeline("2/5").outputs(args.frames) if t), "upsample_rate_3": 2 * (args.frames - 1)}
            def run_leg(name):          # the clock starts with the files open
                vi_leg, rate = legs[name]
                with V.Y4MReader(src) as r, V.Y4MWriter.like(os.devnull, r, rate=rate) as w:
                    t0 = time.perf_counter()
                    vi_leg.run(r, w)
                    w.f.flush()
                    return time.perf_counter() - t0

            secs = timed_legs(legs, run_leg, args.runs, warmup=2, between=share_streams([vi_leg for vi_leg, _ in legs.values()]))
            res["timeline_fps"] = {}
            for name, ts in secs.items():
                v = per_s(synth[name], ts)
                res["timeline_fps"][name] = {"synthesised_frames_per_s": v["median"], "min": v["min"], "max": v["max"],
                                             "synthesised_frames": synth[name]}
            res["timeline_fps"]["note"] = ("both legs run two times per pair on every pair of the clip, 2 streams x 1 pair, file to /dev/null, "
                                           "in turns, on the same two HIP streams; frames that pass through as input bytes are written but not counted")
        if not args.skip_png:
            import visualize_interpolation as viz
            from PIL import Image
            n_png = args.png_frames or args.frames
            png_dir, out_dir = os.path.join(tmp, "png_in"), os.path.join(tmp, "png_out")
            os.makedirs(png_dir)
            for i in range(n_png):
                Image.fromarray(rgb[i].numpy()).save(os.path.join(png_dir, "f_%05d.png" % i))
            ini = os.path.join(tmp, "cfg.ini")
            with open(ini, "w") as f:
                cfg.write(f)
            argv = ["-c", ini, "--expt", "bench", "--log", os.path.join(tmp, "log.txt"), "--input_dir", png_dir, "--img_type", "png",
                    "--upsample_rate", str(RATE), "--output_dir", out_dir]
            model._drop_plans()
            torch.cuda.empty_cache()
            t0 = time.perf_counter()
            k = viz.main(argv, model=model)
            dt = time.perf_counter() - t0
            res["png_fps"] = {"frames_per_s": round(k / dt, 2), "frames_written": k, "input_frames": n_png, "seconds": round(dt, 2),
                              "note": "scripts/visualize_interpolation.py main() on the clip's frames as PNG files, plans built inside the timed call"}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
