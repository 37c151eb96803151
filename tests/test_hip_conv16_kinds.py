"""Every tile kind of the fp16 / fp8 convolution family (csrc/ssm_conv16.hip) in every operand mode, each at the smallest shapes that reach
its decisions: the 9 plain kinds and the 4 fused-upsample kinds x {split, fast, Q8}, cases from tests/hl8_refs.py (a map smaller than a
tile with H = 1 / W = 1, one tile + a one-pixel ragged tile, Cout ragged against BN, the bare Cout = 5, one / two / three 16-channel
chunks (deep kinds: 128, 144), two sources with a batch-broadcast second and a channel-group window as first).

Every case asserts the kind ssm_conv16_plan reports BEFORE it launches: a change of pick16() fails here instead of rerouting the case.

Two checks per case:
  exact   activations and filters in {-1, 0, 1} (fused upsample: activations in {-16, 0, 16}, whose bilinear x2 is an integer in [-16, 16]),
          integer bias, no activation: every product, every fp32 partial sum in any order and every output is an integer below 2048
          (asserted on the reference), so hi holds it exactly, lo and the fp8 compensation terms are zero and all three modes must give
          the float64 convolution BIT FOR BIT - fp32 output, HL8 / Q8 output (decoded here from the raw bytes) and the fused 2x2 mean (a
          multiple of 1/4: exact in hi + lo; mode fast stores fp16 of it, Q8 hi + e4m3 of the rest - the host model of hl8_refs).  One case
          per kind repeats with LeakyReLU slope 0.5 (half-integers, still exact).  A dropped or swapped tap of one channel changes an output
          by an integer: tests/test_conv16_kinds_cpu.py shows the same fault passing the 2e-2 bar of mode fast on random data.
          (The issue proposed filters in {-1, 0, 1} / 16 for the fused upsample; the outputs are then multiples of 1/16 up to ~1000, which
          fp16 does not hold, so mode fast's hi-only output could not be exact.  Filters in {-1, 0, 1} keep every output an integer.)
  random  randn data against oracle.ssm_oracle at the bars of tests/test_hip_conv16.py / tests/test_hip_conv16_q8.py: 5e-5 split, 2e-2 fast,
          1.5e-4 Q8 (Q8 inputs made representable by a load / to_nchw round trip).

Both: outputs pre-filled with NaN and finite afterwards, the zero frame of the HL8 / Q8 output and of the pooled output untouched on both
planes, and mode fast's lo plane still zero.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hl8_refs as L  # noqa: E402

pytestmark = pytest.mark.gpu
NAN16 = 0x7f7f          # an fp16 NaN whose two bytes are e4m3 NaNs


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def hb():
    from ssm_amd import hipbind
    hipbind.load()
    assert (hipbind.SSM_PADY, hipbind.SSM_PADX) == (L.PADY, L.PADX)
    return hipbind


def _load(hb, dev, x, q8, window):
    """(HPlanes, view kwargs, what the kernel reads back as fp32): window = x sits in channel groups 2.. of a tensor with 16 channels of
    noise on either side."""
    if not window:
        p = hb.HPlanes(*x.shape, dev, q8=q8).load(x.to(dev))
        return p, {}, p.to_nchw().cpu()
    B, C, h, w = x.shape
    g = torch.Generator().manual_seed(C + h + w)
    wide = torch.cat([torch.randn(B, 16, h, w, generator=g) * 4, x, torch.randn(B, 16, h, w, generator=g) * 4], 1)
    p = hb.HPlanes(B, C + 32, h, w, dev, q8=q8).load(wide.to(dev))
    return p, {"g0": 2}, p.to_nchw().cpu()[:, 16:16 + C]


def _poisoned(hb, dev, B, C, H, W, mode):
    """An output tensor whose interior is NaN (mode fast: the hi plane only - its lo plane must stay zero)."""
    p = hb.HPlanes(B, C, H, W, dev, q8=mode == "q8")
    v = p.buf[:B * p.G * 2 * p.Hp * p.Wp * 8].view(B, p.G, 2, p.Hp, p.Wp, 8).view(torch.int16)
    v[:, :, 0 if mode == "fast" else slice(None), L.PADY:L.PADY + H, L.PADX:L.PADX + W] = NAN16
    return p


def run(hb, dev, case, mode, a, b, w, bias, lrelu, slope):
    """Launch one problem.  Returns (fp32 output, decoded HL8 / Q8 output or None, decoded pooled output or None, what the kernel read)."""
    q8, fast, cout = mode == "q8", mode == "fast", case.cout_for(mode)
    B, H, W = case.B, case.H, case.W
    pk = hb.PackedConv16(w.to(dev), bias.to(dev), W, q8=q8, ups=case.ups)
    kind, bn, kys = hb.conv16_plan(case.k, case.cin, cout, W, ups=case.ups, q8=q8, fast=fast)
    assert kind == case.kind, "%s runs %s" % (case.id, kind)
    assert bn == pk.bn and (kys == pk.kys or (case.ups and not q8)), (bn, kys, pk.bn, pk.kys)     # HL8 packing does not depend on KYS
    pa, kwa, ra = _load(hb, dev, a, q8, case.window)
    pb, _, rb = _load(hb, dev, b, q8, False) if b is not None else (None, None, None)
    read = ra if b is None else torch.cat([ra, rb.expand(B, -1, -1, -1)], 1)
    y32 = torch.full((B, cout, H, W), float("nan"), device=dev)
    has16 = cout % (16 if q8 else 8) == 0
    dst = _poisoned(hb, dev, B, cout, H, W, mode) if has16 else None
    pool = _poisoned(hb, dev, B, cout, H // 2, W // 2, mode) if has16 and case.pooled() else None
    vb = pb.view(broadcast=case.bcast) if pb else None
    if case.ups:
        hb.conv2d_ups_hl8(pa.view(**kwa), case.c1, vb, case.c2, pk, dst.view() if dst else None, hb.view_of(y32), B, H, W, lrelu=lrelu,
                          slope=slope, fast=fast)
    else:
        hb.conv2d_hl8(pa.view(**kwa), case.c1, vb, case.c2, pk, dst.view() if dst else None, hb.view_of(y32), pool.view() if pool else None,
                      B, H, W, lrelu=lrelu, slope=slope, fast=fast)
    torch.cuda.synchronize()
    got = y32.cpu()
    assert bool(torch.isfinite(got).all()), "fp32 output not finite (or not written)"
    dec = []
    for p, hh, ww, name in ((dst, H, W, "output"), (pool, H // 2, W // 2, "pooled output")):
        if p is None:
            dec.append(None)
            continue
        pl = L.planes(p)
        assert not bool(L.frame_of(pl, hh, ww).any()), "%s: zero frame written" % name
        if fast:
            assert not bool(pl[:, :, 1].view(torch.int16).any()), "%s: mode fast wrote the lo plane" % name
        d = L.decode(pl, q8, cout, hh, ww)
        assert bool(torch.isfinite(d).all()), "%s: not finite (or not written)" % name
        dec.append(d)
    return got, dec[0], dec[1], read


def stored(mode, ref):
    """What a mode's HL8 / Q8 tensor holds of an exactly computed fp32 value."""
    if mode == "split":
        return ref
    return ref.float().half().double() if mode == "fast" else L.q8_model(ref)


_params = [pytest.param(c, m, id="%s-%s" % (c.id, m)) for c in L.ALL_CASES for m in L.MODES]


@pytest.mark.parametrize("case,mode", _params)
def test_conv16_kind_exact_integers(dev, hb, case, mode):
    a, b, cat, w, bias = L.exact_inputs(case, mode)
    for lrelu in ((False, True) if case.slope_half else (False,)):
        want, wpool, premax = L.conv_exact(case, cat, w, bias, lrelu=lrelu, slope=0.5)
        assert premax < 2048, premax
        got, d16, dpool, _ = run(hb, dev, case, mode, a, b, w, bias, lrelu, 0.5)
        bad = int((got.double() != want).sum())
        print("[conv16-kinds] exact  %-44s %-5s %-7s lrelu=%d  max|y| %4d  wrong entries %d" % (case.id, mode, case.kind, lrelu, premax, bad))
        assert torch.equal(got.double(), want), "fp32 output: %d wrong, largest %g" % (bad, float((got.double() - want).abs().max()))
        if d16 is not None:
            assert torch.equal(stored(mode, want), want), "the reference left the exact regime"
            assert torch.equal(d16, want), "HL8 / Q8 output: largest %g" % float((d16 - want).abs().max())
        if dpool is not None:
            assert torch.equal(dpool, stored(mode, wpool)), "pooled output: largest %g" % float((dpool - wpool).abs().max())


@pytest.mark.parametrize("case,mode", _params)
def test_conv16_kind_random_vs_oracle(dev, hb, case, mode):
    from oracle import ssm_oracle as O
    a, b, cat, w, bias = L.random_inputs(case, mode)
    lrelu = case.cout_for(mode) % 8 == 0                     # the bare Cout = 5 is final_conv: no activation
    got, d16, dpool, read = run(hb, dev, case, mode, a, b, w, bias, lrelu, 0.1)
    x = read if mode == "q8" else cat                        # Q8: the representable inputs the kernel read
    x = O.upsample2x_bilinear(x) if case.ups else x
    want = O.conv2d_lrelu(x, w, bias) if lrelu else O.conv2d(x, w, bias)
    errs = [float((got - want).abs().max())]
    if d16 is not None:
        errs.append(float((d16 - want.double()).abs().max()))
    if dpool is not None:
        errs.append(float((dpool - O.avg_pool2(want).double()).abs().max()))
    print("[conv16-kinds] random %-44s %-5s %-7s err fp32 %.2e  16-bit %s  pooled %s  bar %.1e"
          % (case.id, mode, case.kind, errs[0], "%.2e" % errs[1] if d16 is not None else "-", "%.2e" % errs[-1] if dpool is not None else "-",
             L.BARS[mode]))
    assert max(errs) < L.BARS[mode], errs
