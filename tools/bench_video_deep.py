"""The 4:2:2 and 10-bit formats of the streamed video path (ssm_amd.video) on a synthetic 1280x720 clip: one JSON line with
  kernels      event-timed calls on 7 frames of ssm_frames_from_yuvx_fwd / ssm_frames_to_yuvx_fwd for 420p10, 422p10 and 422 beside the 8-bit
               4:2:0 calls (420jpeg, through the same entry points at sample_bytes = 1) and, per call, a device-to-device copy of the bytes
               the call touches once (payload + fp32 planes), in the same run: median over `--windows` windows of `--iters` back-to-back
               calls, per call, and the call's time over its copy's
  stream_fps   output frames per second of VideoInterpolator (upsample_rate 8, 2 streams x 1 pair, file to /dev/null, plans warm) on the clip
               as 420jpeg and as 422p10, run in turns in one process on the same two HIP streams: median and (min, max) over `--runs` runs
`--formats 420jpeg` with `--skip-kernels` is the stream of tools/bench_video.py alone: run from two checkouts in turns it compares a
branch with its parent (`--pkg` names the package directory to import, so that one copy of this tool serves both; a package without the
extended formats runs its 8-bit path).
Usage: python tools/bench_video_deep.py [--frames 41] [--iters 20] [--windows 7] [--runs 3] [--skip-kernels] [--skip-stream]
[--formats 420jpeg,422p10] [--pkg DIR]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

from video_bench import PKG, ROOT, call_ms          # it also puts this checkout's package on the path: main() takes that off again

H, W, RATE = 720, 1280, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=41)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--skip-stream", action="store_true")
    ap.add_argument("--formats", default="420jpeg,422p10", help="the stream's formats, in the order of a turn")
    ap.add_argument("--pkg", default=os.path.join(ROOT, "superslomo-videointerpolation-pytorch_amd"), help="the package directory to import")
    args = ap.parse_args()
    assert 2 <= args.frames <= 43, "synthetic_frames_u8 holds 43 frames of this size at the most"
    # --pkg alone is the package on the path: a module the other checkout lacks is an ImportError, never this checkout's copy
    sys.path[:] = [p for p in sys.path if p not in (PKG, os.path.join(PKG, "scripts"))]
    for p in (ROOT, args.pkg, os.path.join(args.pkg, "scripts")):
        sys.path.insert(0, p)
    import torch
    from models.superslomo_r import FullModel
    from ssm_amd import frames as F
    from ssm_amd import video as V
    from ssm_amd.config import load_config, synthetic_weight_overrides
    from ssm_amd.weights import synthetic_frames_u8, synthetic_state_dict

    extended = hasattr(V, "EXTENDED_TAGS")
    tags = dict(V.EXTENDED_TAGS) if extended else {t: (lay, 8) for t, lay in V.CHROMA_TAGS.items()}
    fmt_kw = (lambda bits: {"bits": bits}) if extended else (lambda bits: {})
    dev = torch.device("cuda:0")
    cfg = load_config("superslomo_original.ini", synthetic_weight_overrides())
    matrix, crange = V.default_matrix(H), V.LIMITED
    rgb = synthetic_frames_u8(args.frames, H, W, seed=42).permute(0, 2, 3, 1).contiguous()          # [n,H,W,3] uint8, host

    def payloads_of(tag, count):
        layout, bits = tags[tag]
        return torch.cat([V.frames_to_yuv(F.frames_from_u8(rgb[i:min(i + 8, count)].to(dev), cfg, True), H, W, layout, matrix, crange, cfg, **fmt_kw(bits)).cpu()
                          for i in range(0, count, 8)]).numpy()

    res = {"clip": {"frames": args.frames, "height": H, "width": W, "upsample_rate": RATE}, "package": os.path.abspath(args.pkg)}
    if not args.skip_kernels:
        n = 7
        (hp, wp), _ = F.padded_dims(H, W)
        x = F.frames_from_u8(rgb[:n].to(dev), cfg, True)
        planes = torch.empty_like(x)
        rec = {"frames": n}
        for tag in ("420jpeg", "420p10", "422p10", "422"):
            layout, bits = tags[tag]
            kw = fmt_kw(bits)
            yuv = torch.from_numpy(payloads_of(tag, n)).to(dev)
            codes = torch.empty_like(yuv)
            sizes = {"from": yuv.numel() + n * 3 * hp * wp * 4, "to": yuv.numel() + n * 3 * H * W * 4}
            calls = {"from": lambda: V.frames_from_yuv(yuv, H, W, layout, matrix, crange, cfg, True, out=planes, **kw),
                     "to": lambda: V.frames_to_yuv(x, H, W, layout, matrix, crange, cfg, out=codes, **kw)}
            rec[tag] = {"bytes_per_pixel_of_payload": round(yuv.numel() / (n * H * W), 2)}
            for side in ("from", "to"):
                half = sizes[side] // 2          # a copy reads and writes: half the bytes moved each way touch the call's bytes once
                a, b = torch.empty(half, dtype=torch.uint8, device=dev), torch.empty(half, dtype=torch.uint8, device=dev)
                ms, copy_ms = call_ms(calls[side], args.iters, args.windows), call_ms(lambda: b.copy_(a), args.iters, args.windows)
                rec[tag]["ssm_frames_%s_yuvx_fwd" % side] = {"ms": round(ms, 4), "one_touch_bytes": sizes[side], "copy_ms": round(copy_ms, 4),
                                                             "ratio_to_copy": round(ms / copy_ms, 2)}
                del a, b
        rec["note"] = ("per call on 7 frames of 720x1280 (canvas 736x1280) into given outputs; the copy moves the call's one-touch bytes "
                       "(reads half, writes half) device to device; a window holds each call's host work too")
        res["kernels"] = rec
        del x, planes

    if not args.skip_stream:
        model = FullModel(cfg)
        model.stage1_model.load_state_dict(synthetic_state_dict(1))
        model.stage2_model.load_state_dict(synthetic_state_dict(2))
        model = model.to(dev).eval()
        formats = [t for t in args.formats.split(",") if t]
        with tempfile.TemporaryDirectory(prefix="bench_video_deep_") as tmp:
            legs = {}
            for tag in formats:
                src = os.path.join(tmp, tag + ".y4m")
                with V.Y4MWriter(src, W, H, rate=(30, 1), aspect=(1, 1), chroma=tag, **({"extended": True} if extended else {})) as wr:
                    for p in payloads_of(tag, args.frames):
                        wr.write_frame(p)
                legs[tag] = (src, V.VideoInterpolator(model, cfg, upsample_rate=RATE, n_streams=2, pairs_per_batch=1))
            fps = {tag: [] for tag in legs}
            for turn in range(args.runs + 2):          # turn 0: plans, pinned buffers' first touch; turn 1: the first run on the shared streams
                if turn == 1 and len(legs) > 1:
                    pipes = [vi._pipe[1] for _, vi in legs.values()]          # every leg on the same two HIP streams
                    for pipe in pipes[1:]:
                        pipe.streams = pipes[0].streams
                for tag, (src, vi) in legs.items():
                    with V.Y4MReader(src, **({"extended": True} if extended else {})) as r, \
                            V.Y4MWriter.like(os.devnull, r, rate=V.output_rate(r.rate, RATE)) as w:
                        t0 = time.perf_counter()
                        k = vi.run(r, w)
                        w.f.flush()
                        dt = time.perf_counter() - t0
                    if turn > 1:
                        fps[tag].append(k / dt)
            res["stream_fps"] = {tag: {"frames_per_s": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2),
                                       "runs": [round(f, 2) for f in v]} for tag, v in fps.items()}
            res["stream_fps"]["note"] = "output frames (originals included) per second of wall time of VideoInterpolator.run, file to /dev/null"
    print(json.dumps(res))


if __name__ == "__main__":
    main()
