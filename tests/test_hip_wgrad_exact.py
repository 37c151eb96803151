"""The three weight-gradient kernels of the training step, held to BIT EQUALITY with float64 autograd in a regime where fp32 is exact.

Kernels: ssm_conv2d_wgrad / ssm_conv2d_wgrad_bias (fp32 MFMA, csrc/ssm_bwd.hip wgrad_mfma_kernel), ssm_conv2d_wgrad_bf16x3 (same file)
and ssm_conv2d_wgrad_wino + ssm_wgrad_wino_finish (csrc/ssm_wgradw.hip) - what autograd computes for nn.Conv2d.weight / .bias of
scripts/models/layers.py:21-33.

The exact regime.  x and dZ are integer-valued fp32, uniform on {-3..3} (seeded).  Every product is an integer of magnitude <= 9 and
every partial sum, in any order, an integer below 9 B H W < 1.1e5 < 2^24: each fp32 MFMA accumulate and each fp32 atomic add is exact, so
the result cannot depend on the summation order, the split over workgroups or the order of the atomics.  The same values are exact in
bf16 (hi = value, lo = 0), so the split-bf16 kernel must give the same bits.  In the Winograd domain B^T x B and A dZ A^T have entries
0, +-1 (integers, |.| <= 12 each, products <= 144, sums < 2^22) and G^T dU G has entries 1, +-1/2: multiples of 1/4, exact as well.
Reference: float64 CPU autograd of oracle.ssm_oracle.conv2d cast to fp32 (train_refs.conv_wgrad_exact, which asserts that the float64
result consists of integers below 2^24).  Comparisons are torch.equal: no tolerance anywhere in this module.

A. ssm_conv2d_wgrad: all 18 instantiations (k x ntc x (SEG, RR)), each at a ragged shape (W no multiple of SEG or of 8, H no multiple
of RR).  wgrad_launch: ntc = 2 if Cout > 32 else 1; tiles = ceil((Cin k^2 [+ 1 with bias]) / 256) * ceil(Cout / (32 ntc));
rows = B ceil(H / RR) ceil(W / SEG); split = gridDim.z = min(512 / tiles, rows) ($SSM_WGRAD_TARGET unset: the module asserts it).  In the
nine ntc = 2 cases rows > 512 / tiles and rows % split != 0: workgroups take several and unequal numbers of staging steps (prefetch of
step s + gridDim.z under the MFMAs of step s, both barriers, reuse of the LDS tiles).  test_fp32_case_table asserts this table.

     k  Cin -> Cout (ntc)   B x H x W  (SEG, RR)   tiles split rows | with the bias column: tiles split
     3  256 -> 128  (2)     2 x 31 x 70   (64, 2)    18    28    64  |  20  25      (Cin k^2 = 9 * 256: the bias column has a
     3  256 -> 128  (2)     3 x 41 x 27   (32, 4)    18    28    33  |  20  25       workgroup column of its own)
     3  256 -> 128  (2)     3 x 85 x 11   (16, 8)    18    28    33  |  20  25
     5   64 -> 128  (2)     2 x 41 x 70   (64, 2)    14    36    84  |  14  36
     5   64 -> 128  (2)     3 x 50 x 27   (32, 4)    14    36    39  |  14  36
     5   64 -> 128  (2)     4 x 75 x 13   (16, 8)    14    36    40  |  14  36
     7   32 ->  64  (2)     2 x 81 x 70   (64, 2)     7    73   164  |   7  73
     7   32 ->  64  (2)     4 x 77 x 21   (32, 4)     7    73    80  |   7  73
     7   32 ->  64  (2)     5 x 123 x 9   (16, 8)     7    73    80  |   7  73
     3   40 ->  32  (1)     1 x  9 x 33   (64, 2)     2     5     5  single step (split = rows); Cout in {32, 20, 5}: the co < Cout
     3   40 ->  20  (1)     1 x  7 x 19   (32, 4)     2     2     2  predicates
     3   40 ->   5  (1)     1 x  5 x 11   (16, 8)     2     1     1
     5   40 ->  20  (1)     1 x  9 x 33   (64, 2)     4     5     5
     5   40 ->   5  (1)     1 x  7 x 19   (32, 4)     4     2     2
     5   40 ->  32  (1)     1 x  5 x 11   (16, 8)     4     1     1
     7   40 ->   5  (1)     1 x  9 x 33   (64, 2)     8     5     5
     7   40 ->  32  (1)     1 x  7 x 19   (32, 4)     8     2     2
     7   40 ->  20  (1)     1 x  5 x 11   (16, 8)     8     1     1
   Per case: zero_first = 1 into a buffer of 7.0; zero_first = 0 onto integer contents; the two-source form into a filter with
   cin_total = Cin + 5 (sources [0, h) and [h, Cin) at ci_offset 2 and 2 + h, h k^2 no multiple of the 256-column block, zero_first = 0:
   the filter columns outside [2, 2 + Cin) keep a NaN-payload sentinel bit for bit); ssm_conv2d_wgrad_bias (dW and db_acc += sum dZ onto
   integer contents).
   ssm_conv2d_wgrad_bf16x3: one shape per launch configuration SSM_WGRAD16(KS, TY, SEG, WAN, WBN), all eight, the same checks without
   the bias form (ca = ceil(Cout/32), cb = ceil(Cin/32); total = B ceil(W/SEG) H steps in nsl slices of sps):
     3 40->72 2x19x37 (3,3,32,2,2) total 76 nsl 5 sps 16 (76 % 16 != 0) | 3 40->20 1x9x70 (3,3,64,1,2) | 3 20->40 1x7x33 (3,3,64,2,1)
     3 5->20 1x11x19 (3,3,64,1,1) | 5 40->40 2x19x70 (5,1,64,2,2) total 76 nsl 5 | 5 20->40 1x9x131 (5,1,128,2,1)
     5 20->20 1x13x41 (5,1,128,1,1): Cin, Cout <= 32 | 7 6->20 2x17x41 (7,1,128,1,1) total 34 nsl 3 sps 12 (34 % 12 != 0)
   ssm_conv2d_wgrad_wino + finish: the seven shapes of tests/test_hip_wgradw.py and its two-source case; db_acc; the scratch ends up
   zero; a second pass finished with scale = 0.5 gives exactly 1.5 x.
B. Neighbours: x is a channel slice [c0, c0 + Cin) of a wider Planes whose other channels are NaN, dZ the first Cout (off 32) channels of a
   Planes with NaN above: the ci < Cin / co < Cout predicates, proven - one ragged shape per kernel size, all three kernels.
C. Memory behind the last plane (the style of tests/test_hip_overshoot.py): the tail slack of x, then of dZ, filled with NaN, then 3e30.
   Shapes whose last pixel group overshoots the row (W = 33, 41 at SEG 64; 17 at SEG 32; 9 at SEG 16; k = 3, 5, 7) and W = 40 (W + 8 a
   multiple of 4 and column 8 ngrp - 1 + PAD inside the row) as the control; the Winograd-domain kernel at the 40+ pixel maps it is used for (41 x 41, 40 x 44).

What was found (MI355X).  A and B: every kernel, every case bit-equal - nothing needed a bound.  (Sensitivity, run once by hand: the
2 x 31 x 70 and 5 x 123 x 9 cases with ONE nonzero pixel of dZ's last row zeroed on the GPU side only - 857 / 446 entries differ, by
at most 9 / 6 of a largest entry of 1263 / 1150: bit equality sees a single pixel.)
C: wgrad_mfma_kernel staged activation columns [xs - 4, xs + SEG + 4) under a row predicate only.  The B operand of the last pixel
group reaches column 8 ngrp - 1 + PAD, past the frame: the first floats of the NEXT plane row.  For k = 3 and 5 that row still belongs
to the plane (the frame has SSM_PADY = 3 rows, the kernel reads PAD = 1 or 2 of them), so those runs passed before the fix as well;
for k = 7 the bottom frame row IS the plane's last row and the floats behind it, on the last plane, are the tail slack: with NaN
there the library before the fix returned NaN in dW[:, Cin - 1, 5:7, 4:7] at 1 x 7 x 33 (0 of the zeroed dZ x NaN; the first shape of
the loop - the test stops there; x poisoned with 3e30, and dZ poisoned with either, passed: 0 x 3e30 = 0 and dZ is never read past W).
Now float4s that begin at roundup4(W + SSM_PADX) or beyond - past the plane row - are staged as zeros, for every kernel size.  The bf16x3 kernel (load_x4 masks at W + 4) and the
Winograd-domain one (pieces outside the image come from the zero frame) never depended on that memory."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_refs as R  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC12345        # a NaN with a payload: survives only if nothing is added to it or stored over it


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    assert os.environ.get("SSM_WGRAD_TARGET") is None, \
        "SSM_WGRAD_TARGET is set: the library reads it once per process and the (tiles, split, rows) table of this module assumes 512"
    return torch.device("cuda:0")


# (k, cin, cout, B, H, W)
FP32_MULTI = [(3, 256, 128, 2, 31, 70), (3, 256, 128, 3, 41, 27), (3, 256, 128, 3, 85, 11),
              (5, 64, 128, 2, 41, 70), (5, 64, 128, 3, 50, 27), (5, 64, 128, 4, 75, 13),
              (7, 32, 64, 2, 81, 70), (7, 32, 64, 4, 77, 21), (7, 32, 64, 5, 123, 9)]
FP32_NTC1 = [(3, 40, 32, 1, 9, 33), (3, 40, 20, 1, 7, 19), (3, 40, 5, 1, 5, 11),
             (5, 40, 20, 1, 9, 33), (5, 40, 5, 1, 7, 19), (5, 40, 32, 1, 5, 11),
             (7, 40, 5, 1, 9, 33), (7, 40, 32, 1, 7, 19), (7, 40, 20, 1, 5, 11)]
BF16_CASES = [(3, 40, 72, 2, 19, 37), (3, 40, 20, 1, 9, 70), (3, 20, 40, 1, 7, 33), (3, 5, 20, 1, 11, 19),
              (5, 40, 40, 2, 19, 70), (5, 20, 40, 1, 9, 131), (5, 20, 20, 1, 13, 41), (7, 6, 20, 2, 17, 41)]
WINO_CASES = [(2, 44, 44, 64, 64), (1, 46, 88, 128, 64), (2, 41, 43, 64, 128), (1, 40, 176, 96, 32), (2, 88, 40, 32, 32),
              (1, 44, 52, 40, 72), (3, 48, 48, 256, 64)]          # (B, H, W, cin, cout) of test_wgrad_wino_vs_autograd


def fp32_launch(k, cin, cout, B, H, W, bias=False):
    """(ntc, seg, rr, tiles, split, rows) of wgrad_launch (csrc/ssm_bwd.hip) at the default target of 512 workgroups."""
    ntc = 2 if cout > 32 else 1
    tiles = -(-(cin * k * k + (1 if bias else 0)) // 256) * -(-cout // (32 * ntc))
    seg = 64 if W > 32 else (32 if W > 16 else 16)
    rr = 128 // seg
    rows = B * -(-H // rr) * -(-W // seg)
    return ntc, seg, rr, tiles, max(1, min(512 // tiles, rows)), rows


def bf16_launch(k, cin, cout, B, H, W):
    """((KS, TY, SEG, WAN, WBN), total, nsl, sps) of ssm_conv2d_wgrad_bf16x3's launch."""
    ca, cb = -(-cout // 32), -(-cin // 32)
    if k == 3:
        cfg = (3, 3, 32, 2, 2) if ca >= 2 and cb >= 2 else (3, 3, 64, 1, 2) if cb >= 2 else (3, 3, 64, 2, 1) if ca >= 2 else (3, 3, 64, 1, 1)
    elif k == 5:
        cfg = (5, 1, 64, 2, 2) if ca >= 2 and cb >= 2 else (5, 1, 128, 2, 1) if ca >= 2 else (5, 1, 128, 1, 1)
    else:
        cfg = (7, 1, 128, 1, 1)
    ks, ty, seg, wan, wbn = cfg
    wgs = -(-cb // wbn) * -(-ca // wan) * (ks // ty)
    total = B * -(-W // seg) * H
    nsl = max(1, min(-(-512 // wgs), -(-total // 16)))
    sps = -(-total // nsl)
    return cfg, total, -(-total // sps), sps


def test_fp32_case_table():
    """The docstring's table: 18 distinct instantiations, ragged shapes, and several unequal steps per workgroup in the ntc = 2 cases
    (with and without the bias column)."""
    seen = set()
    for case in FP32_MULTI + FP32_NTC1:
        k, cin, cout, B, H, W = case
        ntc, seg, rr, tiles, split, rows = fp32_launch(*case)
        seen.add((k, ntc, seg))
        assert W % seg and W % 8 and H % rr, case
        assert B * H * W < 12000
        if case in FP32_MULTI:
            for bias in (False, True):
                _, _, _, t, s, r = fp32_launch(*case, bias=bias)
                assert r > 512 // t and r % s != 0 and s == 512 // t, (case, bias)
    assert len(seen) == 18
    assert any((c[1] * c[0] ** 2) % 256 == 0 for c in FP32_MULTI)          # the bias column in a workgroup column of its own
    cfgs = [bf16_launch(*c) for c in BF16_CASES]
    assert len({c[0] for c in cfgs}) == 8
    assert any(nsl > 1 and total % sps != 0 for _, total, nsl, sps in cfgs)
    assert any(c[0] == 5 and c[1] <= 32 and c[2] <= 32 for c in BF16_CASES)


@functools.lru_cache(maxsize=None)
def _case(k, cin, cout, B, H, W):
    """Inputs and the exact reference of one shape, computed once and shared (never modified) by the tests of all three parts."""
    g = torch.Generator().manual_seed(k * 100003 + cin * 1009 + cout * 101 + B * 31 + H * 7 + W)
    x, dz = R.int_tensor((B, cin, H, W), g), R.int_tensor((B, cout, H, W), g)
    want_w, want_b = R.conv_wgrad_exact(x, dz, k)
    init = R.int_tensor((cout, cin, k, k), g, -50, 50)          # integer contents to accumulate onto
    return x, dz, want_w, want_b, init


def _planes(hb, t, dev, poison=None):
    p = hb.Planes(t.shape[0], t.shape[1], t.shape[2], t.shape[3], dev).load(t.to(dev))
    if poison is not None:
        p.buf[p.full.numel():] = poison          # everything behind the last plane
    return p


def _direct(Bk, xp, dzp, k, dev, split):
    """zero_first = 1 into a buffer of 7.0."""
    dw = torch.full((dzp.C, xp.C, k, k), 7.0, device=dev)
    Bk.wgrad(xp, dzp, dw, k, split=split)
    return dw.cpu()


def _wino(hb, xv, dzv, B, cin, cout, H, W, dev):
    """dW, db and the scratch after ssm_conv2d_wgrad_wino + finish(scale = 1) from zeroed buffers."""
    du, dw, db = torch.zeros(16, cout, cin, device=dev), torch.zeros(cout, cin, 3, 3, device=dev), torch.zeros(cout, device=dev)
    hb.wgrad_wino(xv, dzv, du, db, B, cin, cout, H, W, cin, 0)
    hb.WgradWinoFinish([(du, dw)], dev).run()
    return dw.cpu(), db.cpu(), du


def _check_direct_forms(dev, case, split):
    """zero_first, accumulation and the two-source form of one direct kernel (split: the bf16x3 one), all bitwise."""
    from ssm_amd import backward as Bk
    from ssm_amd import hipbind as hb
    k, cin, cout, B, H, W = case
    x, dz, want_w, want_b, init = _case(*case)
    xp, dzp = _planes(hb, x, dev), _planes(hb, dz, dev)
    assert torch.equal(_direct(Bk, xp, dzp, k, dev, split), want_w), "zero_first = 1 into a buffer of 7.0"
    dw = init.to(dev)
    Bk.wgrad(xp, dzp, dw, k, zero_first=False, split=split)
    assert torch.equal(dw.cpu(), init + want_w), "zero_first = 0 onto integer contents"
    # two sources into a wider filter: columns [2, 2 + cin) of cin + 5, the rest a sentinel that must survive bit for bit
    h = cin // 2 + (3 if cin >= 16 else 1)
    assert 0 < h < cin and (split or (h * k * k) % 256 != 0)
    wide = torch.empty(cout, cin + 5, k, k, device=dev)
    wide.view(torch.int32).fill_(SENTINEL)
    wide[:, 2:2 + cin] = init.to(dev)
    Bk.wgrad(xp.slice(0, h), dzp, wide, k, ci_offset=2, zero_first=False, split=split)
    Bk.wgrad(xp.slice(h, cin - h), dzp, wide, k, ci_offset=2 + h, zero_first=False, split=split)
    wide = wide.cpu()
    assert torch.equal(wide[:, 2:2 + cin], init + want_w), "two sources, zero_first = 0"
    outside = torch.cat([wide[:, :2], wide[:, 2 + cin:]], 1).contiguous().view(torch.int32)
    assert bool((outside == SENTINEL).all()), "filter columns outside [ci_offset, ci_offset + Cin) were touched"
    # ... and with zero_first = 1 on the first source (the whole cin_total-wide filter is zeroed, then both ranges filled)
    wide2 = torch.full((cout, cin + 5, k, k), 7.0, device=dev)
    Bk.wgrad(xp.slice(0, h), dzp, wide2, k, ci_offset=2, zero_first=True, split=split)
    Bk.wgrad(xp.slice(h, cin - h), dzp, wide2, k, ci_offset=2 + h, zero_first=False, split=split)
    full = torch.zeros(cout, cin + 5, k, k)
    full[:, 2:2 + cin] = want_w
    assert torch.equal(wide2.cpu(), full), "two sources, zero_first = 1"
    return xp, dzp


# ---- A. the exact regime ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", FP32_MULTI + FP32_NTC1, ids=lambda c: "k%d_%dto%d_%dx%dx%d" % c)
def test_wgrad_fp32_exact(dev, case):
    from ssm_amd import backward as Bk
    k, cin, cout, B, H, W = case
    xp, dzp = _check_direct_forms(dev, case, split=False)
    _, _, want_w, want_b, init = _case(*case)
    # the bias gradient as one more column of the GEMM: db_acc accumulates exactly sum dZ onto what it held
    db0 = torch.arange(cout, dtype=torch.float32) - 7.0
    dw, db = init.to(dev), db0.to(dev)
    Bk.wgrad(xp, dzp, dw, k, zero_first=False, bias_acc=db)
    assert torch.equal(dw.cpu(), init + want_w), "dW beside the bias column"
    assert torch.equal(db.cpu(), db0 + want_b), "db_acc"
    dw, db = torch.full((cout, cin, k, k), 7.0, device=dev), db0.to(dev)
    Bk.wgrad(xp, dzp, dw, k, zero_first=True, bias_acc=db)
    assert torch.equal(dw.cpu(), want_w) and torch.equal(db.cpu(), db0 + want_b), "zero_first = 1 zeroes dW, never db_acc"


@pytest.mark.parametrize("case", BF16_CASES, ids=lambda c: "k%d_%dto%d_%dx%dx%d" % c)
def test_wgrad_bf16x3_exact(dev, case):
    _check_direct_forms(dev, case, split=True)


@pytest.mark.parametrize("B,H,W,cin,cout", WINO_CASES)
def test_wgrad_wino_exact(dev, B, H, W, cin, cout):
    from ssm_amd import hipbind as hb
    x, dz, want_w, want_b, init = _case(3, cin, cout, B, H, W)
    xp, dzp = _planes(hb, x, dev), _planes(hb, dz, dev)
    du = torch.zeros(16, cout, cin, device=dev)
    db0 = torch.arange(cout, dtype=torch.float32) - 7.0
    dw, db = init.to(dev), db0.to(dev)
    hb.wgrad_wino(xp.view(), dzp.view(), du, db, B, cin, cout, H, W, cin, 0)
    fin = hb.WgradWinoFinish([(du, dw)], dev)
    fin.run()
    assert torch.equal(dw.cpu(), init + want_w), "dW onto integer contents, scale = 1"
    assert torch.equal(db.cpu(), db0 + want_b), "db_acc"
    assert float(du.abs().max()) == 0.0, "the finishing launch leaves the scratch zeroed"
    hb.wgrad_wino(xp.view(), dzp.view(), du, None, B, cin, cout, H, W, cin, 0)
    fin.run(scale=0.5)
    assert torch.equal(dw.cpu(), init + 1.5 * want_w), "second pass, scale = 0.5: exactly 1.5 x"
    assert float(du.abs().max()) == 0.0 and torch.equal(db.cpu(), db0 + want_b)


def test_wgrad_wino_exact_two_sources(dev):
    """cat[a, b] of 32 + 32 channels filled by two launches (the two-source case of tests/test_hip_wgradw.py), one finishing launch."""
    from ssm_amd import hipbind as hb
    B, H, W = 2, 48, 64
    x, dz, want_w, _, _ = _case(3, 64, 32, B, H, W)
    pa, pb, dzp = _planes(hb, x[:, :32], dev), _planes(hb, x[:, 32:], dev), _planes(hb, dz, dev)
    du, dw = torch.zeros(16, 32, 64, device=dev), torch.zeros(32, 64, 3, 3, device=dev)
    hb.wgrad_wino(pa.view(), dzp.view(), du, None, B, 32, 32, H, W, 64, 0)
    hb.wgrad_wino(pb.view(), dzp.view(), du, None, B, 32, 32, H, W, 64, 32)
    hb.WgradWinoFinish([(du, dw)], dev).run()
    assert torch.equal(dw.cpu(), want_w) and float(du.abs().max()) == 0.0


# ---- B. neighbours that must not leak in -----------------------------------------------------------------------------------------
NEIGHBOUR_CASES = [(3, 20, 20, 2, 9, 33), (5, 20, 40, 1, 7, 19), (7, 6, 5, 1, 5, 41)]


def _among_nan(hb, t, c0, extra, dev):
    """Planes of t.C + extra channels, NaN interiors, with t in channels [c0, c0 + t.C): the slice the kernel is given."""
    B, C, H, W = t.shape
    p = hb.Planes(B, C + extra, H, W, dev)
    p.interior[:] = float("nan")
    p.interior[:, c0:c0 + C] = t.to(dev)
    return p.slice(c0, C)


@pytest.mark.parametrize("split", [False, True], ids=["fp32", "bf16x3"])
@pytest.mark.parametrize("case", NEIGHBOUR_CASES, ids=lambda c: "k%d_%dto%d_%dx%dx%d" % c)
def test_nan_in_neighbouring_channels_stays_out(dev, case, split):
    from ssm_amd import backward as Bk
    from ssm_amd import hipbind as hb
    k, cin, cout, B, H, W = case
    assert cout % 32
    x, dz, want_w, want_b, _ = _case(*case)
    xs, dzs = _among_nan(hb, x, 3, 7, dev), _among_nan(hb, dz, 0, 32 - cout % 32, dev)
    assert torch.equal(_direct(Bk, xs, dzs, k, dev, split), want_w)
    if not split:
        dw, db = torch.zeros(cout, cin, k, k, device=dev), torch.zeros(cout, device=dev)
        Bk.wgrad(xs, dzs, dw, k, zero_first=False, bias_acc=db)
        assert torch.equal(dw.cpu(), want_w) and torch.equal(db.cpu(), want_b)


def test_nan_in_neighbouring_channels_stays_out_wino(dev):
    from ssm_amd import hipbind as hb
    k, cin, cout, B, H, W = case = (3, 40, 40, 1, 41, 43)
    x, dz, want_w, want_b, _ = _case(*case)
    xs, dzs = _among_nan(hb, x, 3, 7, dev), _among_nan(hb, dz, 0, 24, dev)
    dw, db, du = _wino(hb, xs.view(), dzs.view(), B, cin, cout, H, W, dev)
    assert torch.equal(dw, want_w) and torch.equal(db, want_b) and float(du.abs().max()) == 0.0


# ---- C. memory behind the last plane ---------------------------------------------------------------------------------------------
SLACK_SHAPES = [(1, 7, 33), (1, 5, 41), (2, 7, 17), (1, 9, 9), (1, 7, 40)]          # SEG 64, 64, 32, 16 and the control (W + 8 = 48)
SLACK_WINO_SHAPES = [(1, 41, 41), (1, 40, 44)]


@pytest.mark.parametrize("poison", [float("nan"), 3.0e30])
@pytest.mark.parametrize("which", ["x", "dz"])
@pytest.mark.parametrize("k", [3, 5, 7])
def test_wgrad_does_not_depend_on_memory_behind_the_last_plane(dev, k, which, poison):
    from ssm_amd import backward as Bk
    from ssm_amd import hipbind as hb
    cin, cout = 6, 8
    for B, H, W in SLACK_SHAPES:
        x, dz, want_w, want_b, _ = _case(k, cin, cout, B, H, W)
        xp = _planes(hb, x, dev, poison if which == "x" else None)
        dzp = _planes(hb, dz, dev, poison if which == "dz" else None)
        for split in (False, True):
            got = _direct(Bk, xp, dzp, k, dev, split)
            name = "%s k%d %dx%dx%d, %s poisoned with %g" % ("bf16x3" if split else "fp32", k, B, H, W, which, poison)
            assert bool(torch.isfinite(got).all()), name + ": non-finite dW at " + str(torch.nonzero(~torch.isfinite(got))[:4].tolist())
            assert torch.equal(got, want_w), name
        dw, db = torch.zeros(cout, cin, k, k, device=dev), torch.zeros(cout, device=dev)
        Bk.wgrad(xp, dzp, dw, k, zero_first=False, bias_acc=db)
        assert torch.equal(dw.cpu(), want_w) and torch.equal(db.cpu(), want_b), "fp32 with the bias column, k%d %dx%dx%d" % (k, B, H, W)


@pytest.mark.parametrize("poison", [float("nan"), 3.0e30])
@pytest.mark.parametrize("which", ["x", "dz"])
def test_wgrad_wino_does_not_depend_on_memory_behind_the_last_plane(dev, which, poison):
    from ssm_amd import hipbind as hb
    cin, cout = 32, 40
    for B, H, W in SLACK_WINO_SHAPES:
        x, dz, want_w, want_b, _ = _case(3, cin, cout, B, H, W)
        xp = _planes(hb, x, dev, poison if which == "x" else None)
        dzp = _planes(hb, dz, dev, poison if which == "dz" else None)
        dw, db, du = _wino(hb, xp.view(), dzp.view(), B, cin, cout, H, W, dev)
        assert bool(torch.isfinite(dw).all()) and bool(torch.isfinite(db).all()), "%dx%d: poison %g reached a sum" % (H, W, poison)
        assert torch.equal(dw, want_w) and torch.equal(db, want_b) and float(du.abs().max()) == 0.0
