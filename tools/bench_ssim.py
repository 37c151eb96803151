"""SSIM and the frame-mix baseline of the hold-out score (ssm_amd/video_score.py) on synthetic frames.  Driver, timers and fixture are
tools/video_bench.py's: three steps, each a child process under its own `timeout`, chained - the first one that fails (or runs into its
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
import os
import statistics
import sys
import tempfile
import time

from video_bench import alternated_ms, drive, parser, per_s, run_only, share_streams, synthetic_model, synthetic_payloads, timed_legs, write_y4m

STEPS = (("kernel_420jpeg", 180), ("kernel_422p10", 180), ("fps", 600))          # step, its time limit in seconds
H, W, HOLD, CLIP_FRAMES = 720, 1280, 8, 65


def call_ms(fn, iters, windows):
    """{median, min, max} of the per-call time in ms of ONE call, its windows back to back: alternated_ms with nothing to alternate with."""
    return alternated_ms({"call": fn}, iters, windows)["call"]


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
    from ssm_amd import video as V
    from ssm_amd import video_score as S
    model, cfg = synthetic_model(dev)
    base = 43          # synthetic_frames_u8 holds 43 frames of this size at the most: the clip plays them forth and back
    made = synthetic_payloads(base, H, W, dev, cfg)
    payloads = made[[i if i < base else 2 * (base - 1) - i for i in range(CLIP_FRAMES)]]
    legs = {"with_ssim_and_mix": S.HoldOutScorer(model, cfg, HOLD, n_streams=2, pairs_per_batch=1, ssim=True, mix=True),
            "without_the_options": S.HoldOutScorer(model, cfg, HOLD, n_streams=2, pairs_per_batch=1)}
    last = {}
    with tempfile.TemporaryDirectory(prefix="bench_ssim_") as tmp:
        full = os.path.join(tmp, "clip.y4m")
        write_y4m(full, payloads, W, H, (240, 1))

        def run(name):          # the clock starts with the files open
            with V.Y4MReader(full) as r, V.Y4MWriter.like(os.devnull, r) as w:
                t0 = time.perf_counter()
                last[name] = legs[name].run(r, w)
                w.f.flush()
                return time.perf_counter() - t0

        secs = timed_legs(legs, run, runs, warmup=2,          # on the streams of the scorer without the options
                          between=share_streams([legs["without_the_options"].vi, legs["with_ssim_and_mix"].vi]))
    on, off = last["with_ssim_and_mix"], last["without_the_options"]
    assert on.frames == off.frames and on.written == off.written == CLIP_FRAMES and len(on.more) == on.scored
    pooled = on.pooled()
    return {"input_frames_read_per_s": {k: per_s(on.frames_read, ts) for k, ts in secs.items()},
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


HEAD = ("SSIM and the frame-mix baseline of the hold-out score (ssm_plane_ssim_fwd, ssm_payload_mix_fwd, HoldOutScorer(ssim=True, mix=True); "
        "DESIGN 3.12).\nOne MI355X, the default precision, synthetic weights and frames.  Tool: tools/bench_ssim.py (each step a process "
        "under its own time limit).\nNothing is asserted; the SSIM and PSNR values of synthetic weights say nothing about quality.\n")


def main():
    args = parser("video_ssim_bench.txt", STEPS).parse_args()
    if args.only:
        return run_only(args.only, lambda: run_step(args.only, args))
    return drive(__file__, HEAD, STEPS, args)


if __name__ == "__main__":
    sys.exit(main())
