"""The training data path (ssm_amd.data, csrc/ssm_data.hip) on a synthetic 1280x720 dataset: one JSON line with
  kernels            event-timed calls of ssm_clip_batch_from_u8_fwd at the config-3 shape (352x352 crops of 720p clips of 3 frames, 2 samples
                     per call and the ini's BATCH_SIZE) beside ssm_frames_from_u8_fwd producing the same number of output bytes from
                     host-cropped frames: median over `--windows` windows of `--iters` back-to-back calls, the one-touch bytes of the call
                     (3 B read + 12 B written per output pixel) and their fraction of the 6.29 TB/s copy ceiling; integer mode, mirrored,
                     and mirrored + rotated
  loader             ClipLoader alone (batches consumed as fast as they come, nothing trained), samples/s per source kind (PNG files,
                     packed .npy clips) and worker count; png_decode_ms is one thread's time to decode one frame
  trainer            Trainer samples/s fed by the loader (PNG and .npy) against the same Trainer fed one resident synthetic batch: the
                     loops alternate in one process after a warm-up, `--runs` runs of `--steps` steps each, median and (min, max)
The dataset (`--clips` distinct clips of 9 frames, each listed `--repeat` times) is written below a temporary directory and deleted afterwards.
Usage: python tools/bench_data.py [--clips 8] [--repeat 8] [--steps 20] [--runs 5] [--iters 20] [--windows 7] [--skip-trainer] [--skip-loader]"""
import argparse
import configparser
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "superslomo-videointerpolation-pytorch_amd")
for p in (ROOT, PKG, os.path.join(PKG, "scripts")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from ssm_amd import data as D  # noqa: E402
from ssm_amd import frames as F  # noqa: E402
from ssm_amd.config import CONFIG_DIR  # noqa: E402
from ssm_amd.weights import synthetic_frames_u8, synthetic_state_dict  # noqa: E402

COPY_CEILING_BYTES_PER_S = 6.29e12
H, W, S, NF = 720, 1280, 352, 9


def call_ms(fn, iters, windows):
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
    return statistics.median(out)


def kernel_record(ms, nbytes):
    ideal_ms = 1e3 * nbytes / COPY_CEILING_BYTES_PER_S
    return {"ms": round(ms, 4), "one_touch_bytes": nbytes, "one_touch_ms": round(ideal_ms, 4), "fraction_of_copy_ceiling": round(ideal_ms / ms, 3)}


def spread(v):
    return {"samples_per_s": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}


def kernel_section(dev, batch, iters, windows):
    rng = np.random.RandomState(1)
    f = 3
    room = f * H * W * 3
    head = 256 * ((batch * 64 + 255) // 256)
    host = rng.randint(0, 256, head + batch * room, dtype=np.uint8)
    inp = torch.empty(batch, 2, 3, S, S, device=dev)
    tgt = torch.empty(batch, 1, 3, S, S, device=dev)
    cropped = torch.from_numpy(rng.randint(0, 256, (batch * f, S, S, 3), dtype=np.uint8)).to(dev)
    one_touch = batch * f * S * S * 15
    rec = {"samples": batch, "output_bytes": batch * f * 3 * S * S * 4,
           "ssm_frames_from_u8_fwd": kernel_record(call_ms(lambda: F.frames_from_u8(cropped), iters, windows), one_touch)}
    for name, flags in (("integer", 0), ("hflip", D.HFLIP), ("hflip_affine", D.HFLIP | D.AFFINE)):
        table = np.zeros(batch, D.RECORD)
        for b in range(batch):
            table[b]["offset"], table[b]["hs"], table[b]["ws"], table[b]["flags"] = head + b * room, H, W, flags
            table[b]["y1"], table[b]["x1"] = rng.randint(0, H - S + 1), rng.randint(0, W - S + 1)
            table[b]["a"] = D.rotation_inverse(rng.randint(0, S), rng.randint(0, S), rng.uniform(-5, 5))
        host[:table.nbytes] = table.view(np.uint8)
        staging = torch.from_numpy(host).to(dev)
        rec["ssm_clip_batch_from_u8_fwd " + name] = kernel_record(call_ms(lambda: D.clip_batch_from_u8(staging, table, inp, tgt), iters, windows), one_touch)
    rec["note"] = "per call; the sibling allocates its output and reads contiguous crops, the new kernel gathers its crops from whole 720p frames"
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=8)
    ap.add_argument("--repeat", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--skip-loader", action="store_true")
    ap.add_argument("--skip-trainer", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = configparser.RawConfigParser()
    cfg.read(os.path.join(CONFIG_DIR, "superslomo_original.ini"))
    ini_batch = cfg.getint("TRAIN", "BATCH_SIZE")
    res = {"dataset": {"clips": args.clips, "listed": args.clips * args.repeat, "frames_per_clip": NF, "height": H, "width": W, "crop": S},
           "kernels": [kernel_section(dev, b, args.iters, args.windows) for b in (2, ini_batch)]}
    tmp = tempfile.mkdtemp(prefix="bench_data_")
    try:
        from PIL import Image
        sys.path.insert(0, os.path.join(PKG, "scripts", "utils"))
        from pack_clips import pack_clips
        lines = []
        for c in range(args.clips):
            fr = synthetic_frames_u8(NF, H, W, seed=300 + c).permute(0, 2, 3, 1).contiguous().numpy()
            os.makedirs(os.path.join(tmp, "c%02d" % c))
            paths = [os.path.join(tmp, "c%02d" % c, "%04d.png" % k) for k in range(NF)]
            for k, p in enumerate(paths):
                Image.fromarray(fr[k]).save(p, compress_level=3)
            lines.append("\n".join(["%d" % NF] + paths))
        png_list, npy_list, once = os.path.join(tmp, "png.txt"), os.path.join(tmp, "npy.txt"), os.path.join(tmp, "once.txt")
        with open(once, "w") as f:
            f.write("\n".join(lines) + "\n")
        with open(png_list, "w") as f:
            f.write("\n".join(lines * args.repeat) + "\n")
        pack_clips(once, os.path.join(tmp, "packed"), os.path.join(tmp, "npy_once.txt"))
        body = open(os.path.join(tmp, "npy_once.txt")).read().split("\n", 1)[1]
        with open(npy_list, "w") as f:
            f.write(body * args.repeat)
        t0 = time.perf_counter()
        for p in D.parse_counted_list(open(once).readlines())[0]:
            D.frame_source(p)
        res["png_decode_ms"] = round(1e3 * (time.perf_counter() - t0) / NF, 2)

        for sec in ("STAGE1", "STAGE2"):
            cfg.set(sec, "LOADPREV", "FALSE")
            cfg.set(sec, "FREEZE", "FALSE")
        cfg.set("DATA", "DATASET", "ADOBE")
        for k, v in (("BATCH_SIZE", 2), ("CROP_IMH", S), ("CROP_IMW", S)):
            cfg.set("TRAIN", k, str(v))

        def loader(kind, workers=None):
            cfg.set("ADOBE_DATA", "TRAINPATHS", png_list if kind == "png" else npy_list)
            return D.ClipLoader(cfg, "TRAIN", dev, 0, 1, seed=1, n_workers=workers)

        if not args.skip_loader:
            rec = {}
            for kind in ("png", "npy"):
                for workers in (1, 4, 12):
                    ld = loader(kind, workers)
                    rates = []
                    for _ in range(3):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        n = sum(x.shape[0] for x, _, _ in ld)
                        torch.cuda.synchronize()
                        rates.append(n / (time.perf_counter() - t0))
                    rec["%s workers=%d" % (kind, ld.n_workers)] = spread(rates[1:])
            rec["note"] = "batches of 2 samples (6 frames of 720p) consumed without training; first epoch dropped (pinned buffers, page cache)"
            res["loader"] = rec

        if not args.skip_trainer:
            from models.superslomo_r import FullModel
            from ssm_amd.training import Trainer
            model = FullModel(cfg)
            model.stage1_model.load_state_dict(synthetic_state_dict(1))
            model.stage2_model.load_state_dict(synthetic_state_dict(2))
            trainer = Trainer(model.to(dev).train(), cfg)
            it = iter(loader("npy"))
            xin, tgt, t = [x.clone() for x in next(it)]
            it.close()
            assert args.steps <= args.clips * args.repeat // 2

            def resident():
                for _ in range(args.steps):
                    yield xin, tgt, t

            def fed(kind):
                ld = loader(kind)

                def gen():
                    for i, b in enumerate(ld):
                        if i == args.steps:
                            return
                        yield b
                return gen

            loops = {"resident": resident, "npy": fed("npy"), "png": fed("png")}
            for g in loops.values():          # warm-up: plans, the recorded step, pinned buffers
                trainer.train(g(), 1)
            rates = {k: [] for k in loops}
            for _ in range(args.runs):
                for k, g in loops.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    n = trainer.train(g(), 1)
                    torch.cuda.synchronize()
                    rates[k].append(2 * n / (time.perf_counter() - t0))
            res["trainer"] = {k: spread(v) for k, v in rates.items()}
            res["trainer"]["note"] = ("%d steps of 2 samples of 352x352 per run, %d runs per loop, alternating; default training precision, no "
                                      "perceptual term; the fed loops include the loader's start-up (first batch decoded inside the timed region)"
                                      % (args.steps, args.runs))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
