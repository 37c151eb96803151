"""The tiled mode (tile = (th, tw): the frame runs in overlapping windows, the windows' frames are stitched on the GPU; an
approximation of the untiled output, not parity) on synthetic frames.  Driver and timer are tools/video_bench.py's; the fps loop, which
builds and frees a pipeline per run, is this tool's own.  Four steps, each a child process under its own `timeout`, chained: the first
one that fails (or runs into its limit) ends the run.  Each step prints one JSON line:
  stitch   event-timed ssm_tile_stitch_fwd over the four tiles of a 2x2 tiling (tile 1088x1920, halo 256, blend 32) of 7 frames at
           2176x3840 - the four launches that stitch one pass - beside a device-to-device copy of the same bytes on the same box:
           median over `--windows` windows of `--iters` back-to-back calls, per call; the one-touch bytes (every pixel of every region of
           influence read once and written once: 24 B per pixel and frame; the read-modify-write of the bands not counted) and their
           fraction of the 6.29 TB/s copy ceiling
  fps      frames per second of PairPipeline.submit in f32w at 2160p (3 streams x 1 pair, 7 times per pair), untiled against
           tile=1088x1920, halo=256; the two settings ALTERNATE, `--runs` runs each (a pipeline is built, warmed, timed and freed per
           run), with the peak device memory of each
  8k       4320x7680 with tile=2176x3840, halo=256, ONE stream: frames per second and peak device memory.  The untiled 8K plan is not
           attempted (scaled from DESIGN 2's figure it does not fit the card); the tiled plan's predicted bytes are asserted against the free memory
           before anything is allocated
  seam     max |difference| and PSNR (denormalised RGB in [0,1]) of tiled against untiled frames at 2160p for halo 64 / 128 / 256 on the
           two synthetic frame families.  With synthetic weights this says how the seam error falls with the halo and nothing about
           visual quality: reported, not asserted
Usage: python tools/bench_tiled.py [--out profiles/tiled_bench.txt] [--only stitch|fps|8k|seam] [--iters 20] [--windows 7] [--runs 3] [--passes 12]"""
import gc
import statistics
import sys
import time

from video_bench import COPY_CEILING_BYTES_PER_S, call_ms, drive, parser, run_only

NT = 7
STEPS = (("stitch", 240), ("fps", 600), ("8k", 420), ("seam", 600))          # step, its time limit in seconds
TILE_4K, TILE_8K, HALO, BLEND = (1088, 1920), (2176, 3840), 256, 32


def bench_stitch(dev, iters, windows):
    import torch
    from ssm_amd import hipbind as hb
    from ssm_amd.tiles import TileGrid
    H, W = 2176, 3840
    g = TileGrid((H, W), TILE_4K, HALO, BLEND)
    assert (g.ny, g.nx) == (2, 2)
    gen = torch.Generator(device="cpu").manual_seed(1)
    tiles = [torch.randn((NT, 3) + g.window, generator=gen).to(dev) for _ in g.tiles]
    out = torch.empty(NT, 3, H, W, device=dev)
    region_px = sum((r[1] - r[0]) * (r[3] - r[2]) for r in map(g.region, g.tiles))

    def stitch():
        for tl, x in zip(g.tiles, tiles):
            hb.tile_stitch(x, out, (tl.y0, tl.x0), (tl.cy0, tl.cx0, tl.cy1, tl.cx1), tl.seams, g.blend)

    nbytes = 24 * NT * region_px
    src, dst = torch.randn(nbytes // 8, device=dev), torch.empty(nbytes // 8, device=dev)          # read nbytes / 2, write nbytes / 2
    ms, copy_ms = call_ms(stitch, iters, windows), call_ms(lambda: dst.copy_(src), iters, windows)
    ideal = 1e3 * nbytes / COPY_CEILING_BYTES_PER_S
    return {"canvas": [H, W], "tile": list(TILE_4K), "halo": HALO, "blend": BLEND, "window": list(g.window), "frames": NT,
            "region_pixels_per_frame": region_px, "canvas_pixels_per_frame": H * W, "one_touch_bytes": nbytes,
            "ssm_tile_stitch_fwd_x4_ms": round(ms, 4), "d2d_copy_same_bytes_ms": round(copy_ms, 4), "one_touch_ms_at_copy_ceiling": round(ideal, 4),
            "stitch_fraction_of_copy_ceiling": round(ideal / ms, 3), "copy_fraction_of_copy_ceiling": round(ideal / copy_ms, 3),
            "stitch_over_copy": round(ms / copy_ms, 3)}


def state_dicts(dev):
    from ssm_amd.weights import synthetic_state_dict
    return ({k: v.to(dev) for k, v in synthetic_state_dict(1).items()}, {k: v.to(dev) for k, v in synthetic_state_dict(2).items()})


def pairs_for(P, H, W, dev, family="texture", seed=42):
    import torch
    from ssm_amd.weights import synthetic_frames
    x = synthetic_frames(P + 1, H, W, seed=seed, family=family)[0].to(dev)
    return torch.cat([x[:-1], x[1:]], 1).contiguous()


def timed_pipeline(dev, sd1, sd2, Hp, Wp, n_streams, passes, tile):
    """(frames per second, peak device memory in bytes) of one pipeline built, warmed, timed and freed."""
    import torch
    from ssm_amd.engine import PairPipeline
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    t = torch.linspace(0.125, 0.875, NT).to(dev)
    pipe = PairPipeline(sd1, sd2, NT, Hp, Wp, dev, True, "f32w", n_streams=n_streams, pairs_per_batch=1, tile=tile, halo=HALO, blend=BLEND)
    img6 = pairs_for(1, Hp, Wp, dev)

    def run(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            pipe.submit(img6, t)
        pipe.sync()
        torch.cuda.synchronize()
        return n * NT / (time.perf_counter() - t0)

    run(2 * n_streams)          # plans, code objects, every slot of the pipeline
    fps = run(passes)
    peak = torch.cuda.max_memory_allocated(dev) - base
    del pipe, img6, run
    gc.collect()
    torch.cuda.empty_cache()
    return fps, peak


def bench_fps(dev, runs, passes):
    from ssm_amd.frames import padded_dims
    sd1, sd2 = state_dicts(dev)
    (Hp, Wp), _ = padded_dims(2160, 3840, 32)
    settings = (("untiled", None), ("tiled", TILE_4K))
    fps, peak = {k: [] for k, _ in settings}, {k: [] for k, _ in settings}
    for _ in range(runs):          # one pipeline alive at a time: three untiled 4K engines take most of the device's memory
        for name, tile in settings:
            f, p = timed_pipeline(dev, sd1, sd2, Hp, Wp, 3, passes, tile)
            fps[name].append(f)
            peak[name].append(p)
    med = {k: statistics.median(v) for k, v in fps.items()}
    rec = {k: {"frames_per_s": [round(v, 2) for v in fps[k]], "median": round(med[k], 2), "peak_device_memory_mib": max(peak[k]) >> 20}
           for k, _ in settings}
    rec["tiled"].update(tile=list(TILE_4K), halo=HALO, blend=BLEND, ratio_to_untiled_median_to_median=round(med["tiled"] / med["untiled"], 3),
                        memory_ratio_to_untiled=round(max(peak["tiled"]) / max(peak["untiled"]), 3))
    rec["note"] = ("interpolated frames per second of wall time at 2160p (canvas %dx%d), PairPipeline f32w, 3 streams x 1 pair, %d times, %d passes "
                   "per run, settings alternated; peak = torch.cuda.max_memory_allocated above the weights, pipeline + one input pair" % (Hp, Wp, NT, passes))
    return rec


PLAN_MARGIN = 1.25          # over DESIGN 2's figure: the untiled 4K pipelines of the `fps` step measure 1.14 times it


def plan_bytes(H, W):
    """Planned need of one PairEngine pass at (H, W): DESIGN 2's 2.2 GB per stage-1 + stage-2 entry at 736x1280 scaled by the pixels, 1 stage-1 +
    NT stage-2 entries per pass (bench.py hbm_needed_bytes), times PLAN_MARGIN."""
    return PLAN_MARGIN * (1 + NT) * 2.2e9 * H * W / (736 * 1280) / 2.0


def predicted_bytes(window, canvas, n_streams=1):
    """Need of a tiled pipeline: per stream the plan of the WINDOW and the full-size output, plus the input pair."""
    return int(n_streams * (plan_bytes(*window) + 4 * 3 * NT * canvas[0] * canvas[1]) + 4 * 6 * canvas[0] * canvas[1])


def bench_8k(dev, passes):
    import torch
    from ssm_amd.tiles import TileGrid
    Hp, Wp = 4320, 7680
    g = TileGrid((Hp, Wp), TILE_8K, HALO, BLEND)
    need = predicted_bytes(g.window, (Hp, Wp))
    untiled = int(plan_bytes(Hp, Wp))
    free_b, total_b = torch.cuda.mem_get_info(dev)
    assert free_b >= need, "%.0f GB of HBM free, the tiled 8K plan needs ~%.0f GB" % (free_b / 1e9, need / 1e9)
    sd1, sd2 = state_dicts(dev)
    fps, peak = timed_pipeline(dev, sd1, sd2, Hp, Wp, 1, passes, TILE_8K)
    return {"canvas": [Hp, Wp], "tile": list(TILE_8K), "halo": HALO, "blend": BLEND, "tiles": [g.ny, g.nx], "window": list(g.window), "streams": 1,
            "frames_per_s": round(fps, 2), "peak_device_memory_mib": peak >> 20, "predicted_need_gb": round(need / 1e9, 1),
            "free_at_start_gb": round(free_b / 1e9, 1), "device_total_gb": round(total_b / 1e9, 1),
            "untiled_plan_predicted_gb_not_attempted": round(untiled / 1e9, 1),
            "note": "one stream x 1 pair, %d times, %d passes; both predictions are DESIGN 2's 2.2 GB per stage-1 + stage-2 entry at 736x1280 scaled by the pixels, "
                    "times %.2f; the untiled one is an extrapolation, not a measurement" % (NT, passes, PLAN_MARGIN)}


def bench_seam(dev):
    import torch
    from ssm_amd.engine import PairPipeline
    from ssm_amd.frames import padded_dims
    from ssm_amd.weights import IMAGENET_MEAN, IMAGENET_STD
    sd1, sd2 = state_dicts(dev)
    (Hp, Wp), _ = padded_dims(2160, 3840, 32)
    t = torch.linspace(0.125, 0.875, NT).to(dev)
    mean = torch.tensor(IMAGENET_MEAN, device=dev).view(1, 3, 1, 1)
    std = torch.tensor(IMAGENET_STD, device=dev).view(1, 3, 1, 1)
    families = ("texture", "edges")
    pairs = {f: pairs_for(1, Hp, Wp, dev, family=f, seed=7) for f in families}
    res = {"canvas": [Hp, Wp], "tile": list(TILE_4K), "blend": BLEND,
           "note": "tiled against untiled frames of the same pair, 7 times, denormalised RGB in [0,1] (max |difference| unclamped, in units of "
                   "full scale); synthetic weights: how the seam error falls with the halo, no statement about visual quality"}
    outs = {}
    for halo in (None, 64, 128, 256):
        pipe = PairPipeline(sd1, sd2, NT, Hp, Wp, dev, True, "f32w", n_streams=1, tile=None if halo is None else TILE_4K, halo=halo or HALO,
                            blend=BLEND)
        for f in families:
            out = pipe.submit(pairs[f], t, clone=True)
            pipe.sync()          # the frames are written on the pipeline's stream: wait before reading them on this one
            torch.cuda.synchronize()
            outs[halo, f] = (out * std + mean).cpu()
            del out
        del pipe
        gc.collect()
        torch.cuda.empty_cache()
    for f in families:
        ref = outs[None, f].double()
        res[f] = {}
        for halo in (64, 128, 256):
            got = outs[halo, f].double()
            mse = ((got.clamp(0, 1) - ref.clamp(0, 1)) ** 2).mean().item()
            res[f]["halo_%d" % halo] = {"max_abs": float("%.3e" % (got - ref).abs().max().item()),
                                        "psnr_db": round(10.0 * torch.log10(torch.tensor(1.0 / max(mse, 1e-30))).item(), 2)}
    return res


def run_step(step, args):
    import torch
    assert torch.cuda.is_available(), "bench_tiled.py measures on the GPU; there is no CPU path"
    dev = torch.device("cuda:0")
    if step == "stitch":
        return bench_stitch(dev, args.iters, args.windows)
    if step == "fps":
        return bench_fps(dev, args.runs, args.passes)
    if step == "8k":
        return bench_8k(dev, args.passes)
    return bench_seam(dev)


HEAD = ("Tiled mode (tile = HxW; DESIGN 3.15) - approximation of the untiled output, not parity.\n"
        "One MI355X, f32w, synthetic weights and frames.  Tool: tools/bench_tiled.py (each step a process under its own time limit).\n")


def main():
    args = parser("tiled_bench.txt", STEPS, passes=12).parse_args()
    if args.only:
        return run_only(args.only, lambda: run_step(args.only, args))
    return drive(__file__, HEAD, STEPS, args)


if __name__ == "__main__":
    sys.exit(main())
