"""SSIM and the frame-mix baseline of the hold-out score (ssm_amd/video_score.py) on synthetic frames, in the manner of
tools/bench_score.py: three steps, each a child process under its own `timeout`, chained - the first one that fails (or runs into its
limit) ends the run.  Each step prints one JSON line:
  kernel_420jpeg, kernel_422p10
           event-timed ssm_plane_ssim_fwd and ssm_payload_mix_fwd on 7 frame pairs at 720p - frames n and n + 1 of 8 payloads in one
           buffer; the mix with k = 1 .. 7 over 8 into a buffer of 7 payloads - beside ssm_plane_sse_fwd ON THE SAME OPERANDS (it reads the
           same samples once: the comparison that matters for the SSIM kernel) and device-to-device copies of the same bytes: one of
           N frame_bytes (the bytes the mix writes; reading and writing together the 2 N frame_bytes the sum kernels read) and one of
           2 N frame_bytes.  Per call: the median over `--windows` windows of `--iters` back-to-back calls, with the least and the largest
           window.  The results are checked against the yardsticks first.
  fps      frames per second of wall time on a 65-frame 720p clip (43 synthetic frames played forth and back), file to /dev/null, in turns
           on the same two HIP streams: HoldOutScorer(hold=8, ssim=True, mix=True) beside HoldOutScorer(hold=8) - the scorer WITHOUT the
           options is the comparison, never the scorer with itself; 2 streams x 1 pair.
Nothing is asserted on the numbers.  With synthetic weights the SSIM values say nothing about quality.
Usage: python tools/bench_ssim.py [--out profiles/video_ssim_bench.txt] [--only STEP] [--iters 20] [--windows 7] [--runs 3]"""
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

STEPS = (("kernel_420jpeg", 180), ("kernel_422p10", 180), ("fps", 600))          # step, its time limit in seconds
H, W, HOLD, CLIP_FRAMES = 720, 1280, 8, 65


def call_ms(fn, iters, windows):
    """{median, min, max} of the per-call time in ms over `windows` event-timed windows of `iters` back-to-back calls."""
    import torch
    for _ in range(5):
        fn()
    out = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / iters)
    return {"median": round(statistics.median(out), 4), "min": round(min(out), 4), "max": round(max(out), 4)}


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
    if bits > 8:          # the clip's significant bits only, as a reader delivers them
        host = torch.from_numpy((host.numpy().view("<u2") & ((1 << bits) - 1)).astype("<u2").view(np.uint8).reshape(n + 1, fb))
    buf = host.to(dev)
    a, b = buf[:-1], buf[1:]
    sums = torch.empty(n, 3, dtype=torch.int64, device=dev)
    mixed = torch.empty(n, fb, dtype=torch.uint8, device=dev)
    nbytes = 2 * n * fb          # what a sum kernel reads; the mix reads 2 payloads (stride 0 on both sides) and writes n
    S.plane_ssim(a, b, H, W, layout, bits, out=sums)
    assert sums.cpu().tolist() == S.plane_ssim_host(host.numpy()[:-1], host.numpy()[1:], H, W, layout, bits).tolist()
    left, right = buf[0:1].expand(n, fb), buf[1:2].expand(n, fb)
    S.payload_mix(left, right, 1, 1, HOLD, bits, out=mixed)
    assert np.array_equal(mixed.cpu().numpy(), S.payload_mix_host(host.numpy()[0:1], host.numpy()[1:2], n, 1, 1, HOLD, bits))
    src, dst = torch.empty(nbytes, dtype=torch.uint8, device=dev).random_(), torch.empty(nbytes, dtype=torch.uint8, device=dev)
    rec = {"pairs": n, "frame": [H, W], "chroma": tag, "frame_bytes": fb, "bytes_read_by_a_sum_kernel": nbytes,
           "windows_per_frame": list(S.plane_windows(H, W, layout)),
           "ssm_plane_ssim_fwd_ms": call_ms(lambda: S.plane_ssim(a, b, H, W, layout, bits, out=sums), iters, windows),
           "ssm_plane_sse_fwd_on_the_same_operands_ms": call_ms(lambda: S.plane_sse(a, b, H, W, layout, bits, out=sums), iters, windows),
           "ssm_payload_mix_fwd_ms": call_ms(lambda: S.payload_mix(left, right, 1, 1, HOLD, bits, out=mixed), iters, windows),
           "ssm_payload_mix_fwd_seven_distinct_pairs_ms": call_ms(lambda: S.payload_mix(a, b, 1, 1, HOLD, bits, out=mixed), iters, windows),
           "d2d_copy_of_N_frame_bytes_ms": call_ms(lambda: dst[:nbytes // 2].copy_(src[:nbytes // 2]), iters, windows),
           "d2d_copy_of_2N_frame_bytes_ms": call_ms(lambda: dst.copy_(src), iters, windows)}
    rec["ssim_over_sse"] = round(rec["ssm_plane_ssim_fwd_ms"]["median"] / rec["ssm_plane_sse_fwd_on_the_same_operands_ms"]["median"], 3)
    rec["mix_over_copy_of_N_frame_bytes"] = round(rec["ssm_payload_mix_fwd_ms"]["median"] / rec["d2d_copy_of_N_frame_bytes_ms"]["median"], 3)
    return rec


def bench_fps(dev, runs):
    import torch
    from models.superslomo_r import FullModel
    from ssm_amd import frames as F
    from ssm_amd import video as V
    from ssm_amd import video_score as S
    from ssm_amd.config import load_config, synthetic_weight_overrides
    from ssm_amd.weights import synthetic_frames_u8, synthetic_state_dict
    cfg = load_config("superslomo_original.ini", synthetic_weight_overrides())
    model = FullModel(cfg)
    model.stage1_model.load_state_dict(synthetic_state_dict(1))
    model.stage2_model.load_state_dict(synthetic_state_dict(2))
    model = model.to(dev).eval()
    base = 43          # synthetic_frames_u8 holds 43 frames of this size at the most: the clip plays them forth and back
    rgb = synthetic_frames_u8(base, H, W, seed=42).permute(0, 2, 3, 1).contiguous()
    matrix, crange, siting = V.default_matrix(H), V.LIMITED, V.CENTRED
    made = torch.cat([V.frames_to_yuv(F.frames_from_u8(rgb[i:i + 8].to(dev), cfg, True), H, W, siting, matrix, crange, cfg).cpu()
                      for i in range(0, base, 8)]).numpy()
    payloads = made[[i if i < base else 2 * (base - 1) - i for i in range(CLIP_FRAMES)]]
    legs = {"with_ssim_and_mix": S.HoldOutScorer(model, cfg, HOLD, n_streams=2, pairs_per_batch=1, ssim=True, mix=True),
            "without_the_options": S.HoldOutScorer(model, cfg, HOLD, n_streams=2, pairs_per_batch=1)}
    secs, last = {k: [] for k in legs}, {}
    with tempfile.TemporaryDirectory(prefix="bench_ssim_") as tmp:
        full = os.path.join(tmp, "clip.y4m")
        with V.Y4MWriter(full, W, H, rate=(240, 1), aspect=(1, 1), chroma="420jpeg") as wr:
            for p in payloads:
                wr.write_frame(p)
        for turn in range(runs + 2):          # turn 0: plans, pinned buffers' first touch; turn 1: the first run on the shared streams
            if turn == 1:
                legs["with_ssim_and_mix"].vi._pipe[1].streams = legs["without_the_options"].vi._pipe[1].streams
            for name, scorer in legs.items():
                with V.Y4MReader(full) as r, V.Y4MWriter.like(os.devnull, r) as w:
                    t0 = time.perf_counter()
                    last[name] = scorer.run(r, w)
                    w.f.flush()
                    dt = time.perf_counter() - t0
                if turn > 1:
                    secs[name].append(dt)
    on, off = last["with_ssim_and_mix"], last["without_the_options"]
    assert on.frames == off.frames and on.written == off.written == CLIP_FRAMES and len(on.more) == on.scored

    def rate(count, ts):
        v = [count / t for t in ts]
        return {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}

    pooled = on.pooled()
    return {"input_frames_read_per_s": {k: rate(on.frames_read, ts) for k, ts in secs.items()},
            "seconds_per_run": {k: [round(t, 3) for t in ts] for k, ts in secs.items()},
            "with_over_without_time": round(statistics.median(secs["with_ssim_and_mix"]) / statistics.median(secs["without_the_options"]), 4),
            "frames_read": on.frames_read, "scored": on.scored,
            "pooled_synthetic_weights_no_statement_on_quality": {
                "psnr_db": {k: {p: round(v, 3) for p, v in pooled[k].items()} for k in ("model", "nearest", "mix")},
                "ssim": {k: {p: round(v, 6) for p, v in d.items()} for k, d in pooled["ssim"].items()}},
            "note": "%d frames of %dx%d (43 synthetic frames forth and back), hold %d, file to /dev/null, 2 streams x 1 pair, legs in turns on the "
                    "same two HIP streams, %d timed runs each" % (CLIP_FRAMES, W, H, HOLD, runs)}


def run_step(step, args):
    import torch
    assert torch.cuda.is_available(), "bench_ssim.py measures on the GPU; there is no CPU path"
    dev = torch.device("cuda:0")
    return bench_fps(dev, args.runs) if step == "fps" else bench_kernel(dev, step.split("_", 1)[1], args.iters, args.windows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=[s for s, _ in STEPS], default=None, help="run this step in this process (what the driver starts)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "video_ssim_bench.txt"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()
    if args.only:
        print(json.dumps({args.only: run_step(args.only, args)}))
        return 0
    head = ("SSIM and the frame-mix baseline of the hold-out score (ssm_plane_ssim_fwd, ssm_payload_mix_fwd, HoldOutScorer(ssim=True, mix=True); "
            "DESIGN 3.12).\nOne MI355X, the default precision, synthetic weights and frames.  Tool: tools/bench_ssim.py (each step a process "
            "under its own time limit).\nNothing is asserted; the SSIM and PSNR values of synthetic weights say nothing about quality.\n")
    with open(args.out, "w") as f:
        f.write(head)
    for step, limit in STEPS:
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--only", step, "--iters", str(args.iters),
               "--windows", str(args.windows), "--runs", str(args.runs)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        line = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else ""
        with open(args.out, "a") as f:
            f.write("\n== %s: `python tools/bench_ssim.py --only %s` (limit %d s, exit status %d) ==\n" % (step, step, limit, r.returncode))
            if r.returncode == 0:
                f.write(json.dumps(json.loads(line), indent=1) + "\n")
        print("%s: exit status %d %s" % (step, r.returncode, line), flush=True)
        if r.returncode != 0:          # a failure, a fault or a time limit: nothing more is started on the GPU
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
