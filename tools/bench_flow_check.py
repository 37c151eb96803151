"""The flow check of the streamed video path (ssm_flow_consistency_fwd, --flow_check; ssm_amd/flow_eval.py) on synthetic
fields and frames.  Driver, timers and fixture are tools/video_bench.py's: two steps, each a child process under its own `timeout`, chained -
the first one that fails (or runs into its limit) ends the run.  Each step prints one JSON line:
  kernel   event-timed ssm_flow_consistency_fwd on 7 pairs of 720 x 1280 (four fp32 planes a pair, 16 B per pixel and pair, read once;
           the gathers of the other field land in cache), without and with the mask, beside ssm_flow_metrics_fwd on the same fields (the
           seven F01 against a ground truth of as many pixels) and a device-to-device copy of the bytes the call reads, ALTERNATED in one
           run: a round times every call once, window after window.  Per call: the median over `--windows` rounds of `--iters`
           back-to-back calls, with the least and the largest; the bytes read as a fraction of the 6.29 TB/s copy ceiling
           (tools/bench_video.py).  The record and the mask are checked against the yardstick first, on one pair.
  fps      output frames per second of wall time, file to /dev/null, in turns on one box: a 65-frame 720 x 1280 clip (33 moving frames
           there and back) through VideoInterpolator(upsample_rate=8) with flow_check=True and without - 64 pairs, 448 synthesised
           frames either way, byte for byte the same output.
Nothing is asserted on the numbers.  With synthetic weights nothing can be said about quality.
Usage: python tools/bench_flow_check.py [--out profiles/flow_check_bench.txt] [--only STEP] [--iters 20] [--windows 7] [--runs 3]"""
import os
import statistics
import sys
import tempfile
import time

from video_bench import (COPY_CEILING_BYTES_PER_S, alternated_ms, drive, parser, per_s, run_only, synthetic_model, synthetic_payloads,
                         timed_legs, write_y4m)

STEPS = (("kernel", 240), ("fps", 600))          # step, its time limit in seconds
H, W, BASE_FRAMES, PAIRS = 720, 1280, 33, 7


def bench_kernel(dev, iters, windows):
    import numpy as np
    import torch
    from ssm_amd import flow_eval as FE
    gen = torch.Generator(device="cpu").manual_seed(1)
    c = 12.0 * torch.rand(PAIRS, 2, 1, 1, generator=gen) - 6.0          # a motion of up to 6 px per pair under +-0.7 px of grain
    host = torch.cat([c + 1.4 * torch.rand(PAIRS, 2, H, W, generator=gen) - 0.7, -c + 1.4 * torch.rand(PAIRS, 2, H, W, generator=gen) - 0.7], 1)
    flow = host.to(dev)
    record, mask = FE.flow_consistency(flow, H, W, want_mask=True)
    want, want_mask = FE.flow_consistency_host(host[:1].numpy(), 0, 0, H, W)
    got = record[:1].cpu().numpy()
    assert np.array_equal(got[..., :3], want[..., :3]) and np.array_equal(mask[:1].cpu().numpy(), want_mask)
    assert np.all(np.abs(got[..., 3] - want[..., 3]) <= 1e-12 * want[..., 3])
    lib = FE.hb.load()
    ws = torch.empty(lib.ssm_flow_consistency_workspace_bytes(PAIRS, H, W), dtype=torch.uint8, device=dev)
    gt = torch.zeros(PAIRS, H, W, 2, dtype=torch.float32, device=dev)
    nbytes = PAIRS * H * W * 16
    src, dst = torch.empty(nbytes, dtype=torch.uint8, device=dev).random_(), torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def with_mask():
        FE.hb.check(lib.ssm_flow_consistency_fwd(FE.hb.view_of(flow), PAIRS, H, W, 0, 0, FE.FLOW_ALPHA, FE.FLOW_BETA, ws.data_ptr(),
                                                 record.data_ptr(), mask.data_ptr(), FE.hb.stream_ptr()))

    calls = {"ssm_flow_consistency_fwd": lambda: FE.flow_consistency(flow, H, W, out=record, workspace=ws),
             "ssm_flow_consistency_fwd_with_mask": with_mask,
             "ssm_flow_metrics_fwd_on_F01": lambda: FE.flow_metric_sums(flow[:, :2], gt),
             "d2d_copy_of_as_many_bytes_as_are_read": lambda: dst.copy_(src)}
    ms = alternated_ms(calls, iters, windows)
    copy = ms["d2d_copy_of_as_many_bytes_as_are_read"]["median"]
    ideal = 1e3 * nbytes / COPY_CEILING_BYTES_PER_S
    shares = [float(FE.FlowCheck.of(r).score) for r in record.cpu().numpy()]
    rec = {"pairs": PAIRS, "field": [H, W], "bytes_read": nbytes, "mask_bytes_written": PAIRS * 2 * H * W,
           "flow_metrics_reads": PAIRS * H * W * 16, "the_copy_reads_and_writes": nbytes,
           "bytes_read_at_the_copy_ceiling_ms": round(ideal, 4), "scores_of_the_synthetic_fields": [round(s, 4) for s in shares],
           "ms_per_call": ms}
    for k in calls:
        rec[k] = {"fraction_of_copy_ceiling": round(ideal / ms[k]["median"], 3), "over_the_copy": round(ms[k]["median"] / copy, 3)}
    rec["consistency_over_flow_metrics"] = round(ms["ssm_flow_consistency_fwd"]["median"] / ms["ssm_flow_metrics_fwd_on_F01"]["median"], 3)
    return rec


def bench_fps(dev, runs):
    import numpy as np
    from ssm_amd import video as V
    model, cfg = synthetic_model(dev)
    matrix = V.default_matrix(H)
    base = synthetic_payloads(BASE_FRAMES, H, W, dev, cfg)
    clip = np.concatenate([base, base[-2::-1]])          # there and back: 65 frames, neighbours always differ
    assert len(clip) == 65
    legs = ("flow_check_upsample_rate_8_65_frames_720p", "upsample_rate_8_65_frames_720p")
    vis = dict(zip(legs, (V.VideoInterpolator(model, cfg, upsample_rate=8, n_streams=2, pairs_per_batch=1, matrix=matrix, flow_check=True),
                          V.VideoInterpolator(model, cfg, upsample_rate=8, n_streams=2, pairs_per_batch=1, matrix=matrix))))
    count = {}
    with tempfile.TemporaryDirectory(prefix="bench_flow_check_") as tmp:
        path = os.path.join(tmp, "clip.y4m")
        write_y4m(path, clip, W, H, (30, 1))

        def run(name):          # the clock runs while the files are opened and closed
            t0 = time.perf_counter()
            with V.Y4MReader(path) as r:
                with V.Y4MWriter.like(os.devnull, r) as w:
                    count[name] = vis[name].run(r, w)
                    w.f.flush()
            return time.perf_counter() - t0

        secs = timed_legs(legs, run, runs)
    checks = vis[legs[0]].flow_checks
    assert count == {k: 64 * 8 + 1 for k in legs} and [i for i, _ in checks] == list(range(64)) and vis[legs[1]].flow_checks == []
    med = {k: statistics.median(ts) for k, ts in secs.items()}
    scores = sorted(float(c.score) for _, c in checks)
    return {"output_frames_per_s": {k: per_s(count[k], ts) for k, ts in secs.items()},
            "seconds_per_run": {k: [round(t, 3) for t in ts] for k, ts in secs.items()},
            "outputs": count, "pairs": 64, "synthesised": 448,
            "scores_with_the_synthetic_weights": {"min": round(scores[0], 4), "median": round(scores[32], 4), "max": round(scores[-1], 4)},
            "flow_check_over_plain_time_per_run": round(med[legs[0]] / med[legs[1]], 4),
            "spread_of_the_plain_leg": round((max(secs[legs[1]]) - min(secs[legs[1]])) / med[legs[1]], 4),
            "note": "%d moving frames of %dx%d there and back as 65 frames through upsample_rate=8 with flow_check=True and without; file "
                    "to /dev/null, 2 streams x 1 pair, legs in turns, %d timed runs each" % (BASE_FRAMES, W, H, runs)}


def run_step(step, args):
    import torch
    assert torch.cuda.is_available(), "bench_flow_check.py measures on the GPU; there is no CPU path"
    dev = torch.device("cuda:0")
    return bench_fps(dev, args.runs) if step == "fps" else bench_kernel(dev, args.iters, args.windows)


HEAD = ("The flow check of the streamed video path (ssm_flow_consistency_fwd, --flow_check; DESIGN 3.12).\nOne MI355X, the default "
        "precision, synthetic weights, fields and frames.  Tool: tools/bench_flow_check.py (each step a process under its own time limit).\n"
        "Nothing is asserted; with synthetic weights nothing can be said about quality.  No kernel trace was taken.\n")


def main():
    args = parser("flow_check_bench.txt", STEPS).parse_args()
    if args.only:
        return run_only(args.only, lambda: run_step(args.only, args))
    return drive(__file__, HEAD, STEPS, args)


if __name__ == "__main__":
    sys.exit(main())
