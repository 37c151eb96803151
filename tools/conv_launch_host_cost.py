#!/usr/bin/env python3
"""Host cost of one fp32 convolution launch through ssm_amd/hipbind.py.

    python tools/conv_launch_host_cost.py [--tree ROOT] [--label NAME]           on the GPU
    python tools/conv_launch_host_cost.py --stub [--tree ROOT] [--label NAME]    on any host

Without --stub: 20 000 conv2d_wino4 calls (16 -> 32 channels, batch 2, 8x12 map, pooled output) after 2 000 warm-up calls,
time.perf_counter around the loop, no synchronisation inside it, three repeats, microseconds per call.  With --stub: the interpreter's
share alone - the library and the stream lookup are replaced by stubs, so no device is needed - for conv2d_wino4 and for conv2d_wino (plan
check and cached split factor), best of 7 x 200 000 calls.  --tree: the checkout whose binding is measured (default: this one), so that two
trees can be compared from one copy of this file."""
import argparse
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--label", default="tree")
ap.add_argument("--stub", action="store_true")
args = ap.parse_args()
ROOT = os.path.abspath(args.tree)
sys.path[:0] = [ROOT, os.path.join(ROOT, "superslomo-videointerpolation-pytorch_amd")]
import torch  # noqa: E402

from ssm_amd import hipbind as hb  # noqa: E402

assert os.path.abspath(hb.__file__).startswith(ROOT), hb.__file__
B, H, W, CIN, COUT = 2, 8, 12, 16, 32


def per_call(fn, n):
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    return (time.perf_counter() - t0) / n * 1e6


def stubbed():
    class Lib:
        def __getattr__(self, name):
            fn = lambda *a: 0  # noqa: E731
            setattr(self, name, fn)
            return fn

    class Tensor:
        def data_ptr(self):
            return 4096

    hb._lib = Lib()
    hb.stream_ptr = lambda: 7
    hb.wino_plan = lambda *a: (0, 32, 8)
    v = hb.SsmView(4096, 2, 3, 4)
    for name, cls, ck in (("conv2d_wino4", hb.PackedWino4, 4), ("conv2d_wino", hb.PackedWino, 8)):
        pk = cls.__new__(cls)
        pk.w, pk.b, pk.cin, pk.cin_p, pk.cout, pk.k, pk.bn, pk.ck = Tensor(), Tensor(), CIN, CIN, COUT, 3, 32, ck
        pk._splitk = {(B, H, W, False): 1}
        fn = getattr(hb, name)
        best = min(per_call(lambda: fn(v, CIN, None, 0, pk, v, v, B, H, W), 200000) for _ in range(7))
        print("interpreter share %s %s: %.3f us per call" % (args.label, name, best), flush=True)


def on_gpu():
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    pk = hb.PackedWino4((torch.randn(COUT, CIN, 3, 3, generator=g) / 12).to(dev), torch.randn(COUT, generator=g).to(dev), B, H, W, pool=True)
    x = hb.Planes(B, CIN, H, W, dev).load(torch.randn(B, CIN, H, W, generator=g).to(dev))
    y, yp = hb.Planes(B, COUT, H, W, dev), hb.Planes(B, COUT, H // 2, W // 2, dev)
    xv, yv, pv = x.view(), y.view(), yp.view()
    launch = lambda: hb.conv2d_wino4(xv, CIN, None, 0, pk, yv, pv, B, H, W)  # noqa: E731
    per_call(launch, 2000)
    torch.cuda.synchronize()
    for rep in range(3):
        us = per_call(launch, 20000)
        torch.cuda.synchronize()
        print("host_cost %s repeat %d: %.3f us per conv2d_wino4 call" % (args.label, rep + 1, us), flush=True)


if __name__ == "__main__":
    stubbed() if args.stub else on_gpu()
