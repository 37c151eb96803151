"""Per-layer A/B of the decoder's fused-upsample 3x3 layers: today's kernel (what choose_algo picks without the low-res GEMM form) against
GEMM + combine pass (csrc/ssm_upgemm.hip), at the shapes of stage 1 (batch 2), stage 2 (batch 14) and the 4K plan (batch 7).

    python tools/bench_upgemm_layers.py [--rounds 5] [--iters 10] [--plans 720p_s1,720p_s2,4k_s2]

The two forms alternate in one process (rounds x iters launches each, HIP events around each block of iters); the table gives the median and
the spread (min .. max) of the per-launch time over the rounds.  The split of the new form into its two kernels comes from a
`rocprofv3 --kernel-trace` run of this tool (--trace-csv <kernel_trace.csv> prints the median duration per kernel and grid size; the grid
sizes of every case are printed beside it)."""
import argparse
import csv
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "superslomo-videointerpolation-pytorch_amd")):
    sys.path.insert(0, p)

# layer: (C1, C2, Cout, scale of the OUTPUT map, second source batch-broadcast / addend)
LAYERS = {"conv7a": (512, 0, 512, 16), "conv8a": (512, 512, 256, 8), "conv9a": (256, 256, 128, 4), "conv10a": (128, 128, 64, 2),
          "conv11a": (64, 64, 32, 1)}
PLANS = {"720p_s1": (2, 736, 1280), "720p_s2": (14, 736, 1280), "4k_s2": (7, 2176, 3840)}
PEAK = 157.3e12


def trace_table(path):
    rows = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"]
            if "upgemm" not in name and "w4_" not in name and "wino4" not in name:
                continue
            m = re.search(r"(upgemm_\w+|w4_\w+|wino4_\w+)(<[^>]*>+)?", name)
            short = (m.group(0) if m else name)[:60]
            rows.setdefault((short, r.get("Grid_Size", r.get("Grid_Size_X", "?"))), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for (name, grid), d in sorted(rows.items()):
        print("%-62s grid %-10s n %4d  median %9.1f us  min %9.1f" % (name, grid, len(d), statistics.median(d), min(d)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--plans", default="720p_s1,720p_s2,4k_s2")
    ap.add_argument("--layers", default="conv7a,conv8a,conv9a,conv10a")
    ap.add_argument("--trace-csv")
    a = ap.parse_args()
    if a.trace_csv:
        return trace_table(a.trace_csv)
    import torch
    from ssm_amd import engine as E
    from ssm_amd import hipbind as hb
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    print("%-8s %-8s %3s %9s | %-7s %9s %17s | %9s %17s | %7s | %s" % ("plan", "layer", "B", "low-res", "today", "ms", "(min .. max)", "upgemm ms", "(min .. max)",
                                                                     "gain ms", "GEMM grid x256, combine grid x256, GEMM GFLOP, combine MB"))
    for plan in a.plans.split(","):
        B, H0, W0 = PLANS[plan]
        for name in a.layers.split(","):
            c1, c2, cout, s = LAYERS[name]
            H, W = H0 // s, W0 // s
            h, w = H // 2, W // 2
            wt = (torch.randn(cout, c1 + c2, 3, 3, generator=g) / ((c1 + c2) * 9) ** 0.5).to(dev)
            bias = (torch.randn(cout, generator=g) * 0.1).to(dev)
            pa = hb.Planes(B, c1, h, w, dev)
            pa.interior.copy_(torch.randn(B, c1, h, w, generator=g).to(dev))
            pb = None
            if c2:
                pb = hb.Planes(B, c2, h, w, dev)
                pb.interior.copy_(torch.randn(B, c2, h, w, generator=g).to(dev))
            y = hb.Planes(B, cout, H, W, dev)
            algo = E.choose_algo(name, c1 + c2, cout, 3, B, H, W, True, True, True, upgemm=False)
            pk_old = E._ALGO_CLASS[algo]()(wt, bias, B, H, W, ups=True)
            pk_new = hb.PackedUpGemm(wt, bias, B, H, W)
            forms = {"old": (E.conv_fn(pk_old, True), pk_old), "new": (hb.conv2d_ups_upgemm, pk_new)}

            def launch(form):
                fn, pk = forms[form]
                fn(pa.view(), c1, pb.view() if pb else None, c2, pk, y.view(), B, H, W, lrelu=True)
            for form in forms:
                for _ in range(3):
                    launch(form)
            torch.cuda.synchronize()
            times = {"old": [], "new": []}
            for _ in range(a.rounds):
                for form in ("old", "new"):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.iters):
                        launch(form)
                    e1.record()
                    torch.cuda.synchronize()
                    times[form].append(e0.elapsed_time(e1) / a.iters)
            o, n = times["old"], times["new"]
            mo, mn = statistics.median(o), statistics.median(n)
            th, tw = (16, 16) if ((h + 15) // 16 * 16) * ((w + 15) // 16 * 16) <= ((h + 7) // 8 * 8) * ((w + 15) // 16 * 16) else (8, 16)
            ggrid = B * ((h + th - 1) // th) * ((w + tw - 1) // tw) * ((9 * cout + 127) // 128)
            cgrid = (B * cout * h * ((w + 3) // 4) + 255) // 256
            gflop = 2.0 * B * h * w * 9 * cout * (c1 + c2) / 1e9
            cmb = 4.0 * B * cout * h * w * 13 / 1e6
            print("%-8s %-8s %3d %4dx%-4d | %-7s %9.4f (%7.4f..%7.4f) | %9.4f (%7.4f..%7.4f) | %+7.4f | %d, %d, %.1f, %.0f" % (
                plan, name, B, h, w, algo, mo, min(o), max(o), mn, min(n), max(n), mn - mo, ggrid, cgrid, gflop, cmb), flush=True)
            del pa, pb, y, pk_old, pk_new, forms
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
