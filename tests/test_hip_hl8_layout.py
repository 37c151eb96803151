"""The layout, gather and element-wise kernels of the HL8 / Q8 path, each called through the C ABI on its own: the four layout converters
(ssm_hl8_from_f32, ssm_hl8_to_f32, ssm_hq8_from_f32, ssm_hq8_to_f32), ssm_upsample2x_cat_hl8_fwd, ssm_flowinterp_inputs_hl8_fwd /
_hq8_fwd and ssm_hl8_gather_cols.  The fp32 siblings are pinned in tests/test_hip_infer_elementwise.py; same references
(tests/train_refs.py), same yardstick.

HL8 / Q8 buffers are encoded and decoded HERE from the raw bytes (tests/hl8_refs.py, written from the comments of include/ssm_hip.h:
hi + lo, and hi + e4m3(lo * 2^11) * 2^-11 with an explicit e4m3 table), so a decode fault cannot cancel an encode fault.

Bars.  Converters and the gather: bit equality with the host encoding / the source records.  Bilinear x2 on small multiples of 16: equality
with the float64 reference.  On randn data: the fp32 sibling's bar - train_refs.bar(e_ref) = max(8 e_ref, 4 * 2^-24) of the largest
reference entry, e_ref = the fp32 CPU oracle's own distance from the float64 oracle - plus the representation error of the largest
reference entry in the output's format (hl8_refs.rep_error_bound, derived from the formats and checked against the host model in
tests/test_conv16_kinds_cpu.py).  Neither figure comes from a kernel."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hl8_refs as L  # noqa: E402
import train_refs as R  # noqa: E402
from train_refs import Box, dptr  # noqa: E402

pytestmark = pytest.mark.gpu
F64 = torch.float64
NAN = float("nan")


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


def i16(t):
    return t.contiguous().view(torch.int16)


def groups_for(C, q8):
    G = (C + 7) // 8 + 1                     # one group more than the channels need: its channels must come out zero
    return G + (G % 2 if q8 else 0)          # Q8: an odd count rounded up to a pair


# ======================================================================================================================
# layout converters
# ======================================================================================================================
@pytest.mark.parametrize("layout", R.LAYOUTS)
@pytest.mark.parametrize("q8", [False, True], ids=["hl8", "q8"])
@pytest.mark.parametrize("C", [1, 13, 16])
def test_layout_converters_bit_for_bit(dev, hb, C, q8, layout):
    """from_f32: the raw planes equal the host encoding bit for bit - hi = fp16(x), lo = fp16(x - hi) / the two e4m3 planes of a group
    pair - channels C..8G-1 and the frame zero.  to_f32: float(hi) + float(lo) (Q8: + e4m3 * 2^-11) rounded once to fp32, bit for bit,
    from planes encoded on the host.  W in {1, 63, 65} x H in {1, 5} around the 64 x 4 thread blocks; the inputs hold 600 and -1e4
    (beyond e4m3's 448: the fp8 copies saturate, hi stays exact), 0, -0 and values whose lo is a subnormal."""
    lib, st = hb.load(), hb.stream_ptr
    B, G = 2, groups_for(C, q8)
    frm, to = (lib.ssm_hq8_from_f32, lib.ssm_hq8_to_f32) if q8 else (lib.ssm_hl8_from_f32, lib.ssm_hl8_to_f32)
    for H in (1, 5):
        for W in (1, 63, 65):
            g = torch.Generator().manual_seed(C * 100 + H * 10 + W)
            x = torch.randn(B, C, H, W, generator=g) * 3
            flat = x.view(-1)
            for i, v in enumerate((600.0, -1e4, 0.0, -0.0, 2.0 ** -12 + 2.0 ** -24, 1e-6)):
                flat[i::17] = v
            src = Box(hb, dev, layout, x)
            dst = hb.HPlanes(B, C, H, W, dev, groups=G, q8=q8)
            hb.check(frm(src.view(), dst.view(), B, C, G, H, W, st()))
            got, want = L.planes(dst), L.encode(x, G, q8, dst.Hp, dst.Wp)
            bad = i16(got) != i16(want)
            assert not bool(bad.any()), "from_f32 %s C=%d %dx%d: %d halves differ (first at %s)" % (
                "q8" if q8 else "hl8", C, H, W, int(bad.sum()), bad.nonzero()[0].tolist())
            assert not bool(L.frame_of(got, H, W).any())
            # back, from planes the host encoded (of other values), into a NaN-filled output with a canary behind it
            x2 = torch.randn(B, C, H, W, generator=g) * 3
            x2.view(-1)[::13] = 700.0
            pl = L.encode(x2, G, q8, dst.Hp, dst.Wp)
            out = R.plant_canary(Box(hb, dev, layout, shape=(B, C, H, W), fill=NAN))
            enc = hb.HPlanes(B, C, H, W, dev, groups=G, q8=q8)
            enc.buf[:pl.numel()] = pl.reshape(-1).to(dev)
            hb.check(to(enc.view(), out.view(), B, C, G, H, W, st()))
            back = out.get()
            assert bool(torch.isfinite(back).all()) and out.frame_is_zero() and R.canary_intact(out)
            assert torch.equal(R.bits(back), R.bits(L.decode(pl, q8, C, H, W).float())), "to_f32 %s C=%d %dx%d" % (q8, C, H, W)
            assert float((back.double() - x2.double()).abs().max()) <= L.rep_error_bound(float(x2.abs().max()), q8) * (1 + 2.0 ** -20)


# ======================================================================================================================
# concat + bilinear x2
# ======================================================================================================================
def _ups_call(hb, dev, a, b, bcast, Ga, Gb):
    B, _, h, w = a.shape
    pa = hb.HPlanes(B, 8 * Ga, h, w, dev).load(a.to(dev))
    pb = hb.HPlanes(b.shape[0], 8 * Gb, h, w, dev).load(b.to(dev)) if Gb else None
    y = hb.HPlanes(B, 8 * (Ga + Gb), 2 * h, 2 * w, dev)
    v = y.buf[:B * y.G * 2 * y.Hp * y.Wp * 8].view(B, y.G, 2, y.Hp, y.Wp, 8)
    v[:, :, :, L.PADY:L.PADY + 2 * h, L.PADX:L.PADX + 2 * w] = NAN
    hb.check(hb.load().ssm_upsample2x_cat_hl8_fwd(pa.view(), Ga, pb.view(broadcast=bcast) if Gb else hb.NULL_HVIEW, Gb, y.view(), B, h, w,
                                                  hb.stream_ptr()))
    pl = L.planes(y)
    assert not bool(L.frame_of(pl, 2 * h, 2 * w).any()), "wrote into the zero frame"
    got = L.decode(pl, False, 8 * (Ga + Gb), 2 * h, 2 * w)
    assert bool(torch.isfinite(got).all()), "not finite (or not written)"
    # what the kernel read: the sources as HL8 holds them, decoded here
    ra = L.decode(L.planes(pa), False, 8 * Ga, h, w)
    rb = L.decode(L.planes(pb), False, 8 * Gb, h, w).expand(B, -1, -1, -1) if Gb else None
    return got, (ra if rb is None else torch.cat([ra, rb], 1))


@pytest.mark.parametrize("h,w", R.UPSAMPLE_HW, ids=str)
@pytest.mark.parametrize("Ga,Gb", [(1, 0), (2, 1)], ids=str)
def test_upsample2x_cat_hl8(dev, hb, Ga, Gb, h, w):
    """ssm_upsample2x_cat_hl8_fwd against O.upsample2x_bilinear(cat) in float64, the second source batch-broadcast.  Small multiples of 16:
    every product with 1/4 and 3/4 is an integer, hi holds it: equality.  randn: the bar of the module docstring."""
    from oracle import ssm_oracle as O
    B = 2
    g = torch.Generator().manual_seed(Ga * 100 + Gb * 10 + h + w)
    ia = R.int_tensor((B, 8 * Ga, h, w), g) * 16
    ib = R.int_tensor((1, 8 * Gb, h, w), g) * 16 if Gb else None
    got, cat = _ups_call(hb, dev, ia, ib, True, Ga, Gb)
    assert torch.equal(cat, (ia if ib is None else torch.cat([ia, ib.expand(B, -1, -1, -1)], 1)).double())
    assert torch.equal(got, O.upsample2x_bilinear(cat)), "exact inputs: largest %g" % float((got - O.upsample2x_bilinear(cat)).abs().max())
    ra = torch.randn(B, 8 * Ga, h, w, generator=g)
    rb = torch.randn(1, 8 * Gb, h, w, generator=g) if Gb else None
    got, cat = _ups_call(hb, dev, ra, rb, True, Ga, Gb)
    want = O.upsample2x_bilinear(cat)
    e_ref = R.rel_err(O.upsample2x_bilinear(cat.float()), want)
    top = float(want.abs().max())
    bound = R.bar(e_ref) * top + L.rep_error_bound(top, False)
    err = float((got - want).abs().max())
    print("[hl8-layout] upsample2x_cat_hl8 Ga=%d Gb=%d %dx%d: err %.3e  bound %.3e (e_ref %.3e, max|y| %.2f)" % (Ga, Gb, h, w, err, bound, e_ref, top))
    assert err <= bound


# ======================================================================================================================
# the stage-2 input builder
# ======================================================================================================================
def _inputs_hl8(hb, dev, c, q8, layout):
    B, _, H, W = c["img6"].shape
    lib = hb.load()
    img6, flow4 = Box(hb, dev, layout, c["img6"]), Box(hb, dev, layout, c["flow4"])
    flows = R.plant_canary(Box(hb, dev, layout, shape=(B, 4, H, W), fill=NAN))
    out = hb.HPlanes(B, 16, H, W, dev, q8=q8)
    td = c["t"].to(dev)
    fn = lib.ssm_flowinterp_inputs_hq8_fwd if q8 else lib.ssm_flowinterp_inputs_hl8_fwd
    hb.check(fn(img6.view(), flow4.view(), dptr(td), out.view(), flows.view(), B, H, W, hb.stream_ptr()))
    pl = L.planes(out)
    assert not bool(L.frame_of(pl, H, W).any()), "wrote into the zero frame of out16"
    f4 = flows.get()
    assert bool(torch.isfinite(f4).all()) and flows.frame_is_zero() and R.canary_intact(flows)
    return L.decode(pl, q8, 16, H, W), f4


def _check_inputs_hl8(c, got, f4, q8, name):
    want = R.inputs_fwd(c["img6"], c["flow4"], c["t"], F64)
    lo = R.inputs_fwd(c["img6"], c["flow4"], c["t"], torch.float32)
    worst = 0.0
    for grp, a, b in R.INPUT_GROUPS:
        top = float(want[:, a:b].abs().max())
        bound = R.bar(R.rel_err(lo[:, a:b], want[:, a:b])) * top + L.rep_error_bound(top, q8)
        err = float((got[:, a:b] - want[:, a:b]).abs().max())
        worst = max(worst, err / bound)
        print("[hl8-layout] %s %-6s err %.3e  bound %.3e  (max|ref| %.2f)" % (name, grp, err, bound, top))
        assert err <= bound, (name, grp, err, bound)
    # the fp32 flows: channels 6:10 at the fp32 sibling's bar
    e_ref = R.rel_err(lo[:, 6:10], want[:, 6:10])
    err = R.rel_err(f4, want[:, 6:10])
    print("[hl8-layout] %s flows4 err %.3e  e_ref %.3e  bar %.3e;  worst out16 err / bound %.2f" % (name, err, e_ref, R.bar(e_ref), worst))
    assert err <= R.bar(e_ref), (name, err, e_ref)


@pytest.mark.parametrize("layout", R.LAYOUTS)
@pytest.mark.parametrize("q8", [False, True], ids=["hl8", "q8"])
@pytest.mark.parametrize("shape,scale", R.SAMPLER_CASES, ids=str)
def test_flowinterp_inputs_hl8(dev, hb, shape, scale, q8, layout):
    c = R.make_case(shape, scale)
    got, f4 = _inputs_hl8(hb, dev, c, q8, layout)
    _check_inputs_hl8(c, got, f4, q8, "inputs-%s %s x%g %s" % ("q8" if q8 else "hl8", shape, scale, layout))


@pytest.mark.parametrize("q8", [False, True], ids=["hl8", "q8"])
def test_flowinterp_inputs_hl8_at_the_ends_of_the_interval(dev, hb, q8):
    c = R.make_case((3, 9, 70), 3.0)
    c["t"] = torch.tensor([0.0, 1.0, 0.0])
    got, f4 = _inputs_hl8(hb, dev, c, q8, "planes")
    _check_inputs_hl8(c, got, f4, q8, "inputs-%s t-ends" % ("q8" if q8 else "hl8"))
    assert not bool(got[0, 8:10].any()) and not bool(got[1, 6:8].any())          # t = 0: Ft0^ = 0;  t = 1: Ft1^ = 0
    assert not bool(f4[0, 2:4].any()) and not bool(f4[1, 0:2].any())


# ======================================================================================================================
# column gather of the sub-pixel convolution's strips
# ======================================================================================================================
@pytest.mark.parametrize("H", [1, 5, 257])
@pytest.mark.parametrize("Ga,Gb", [(1, 0), (2, 2)], ids=str)
@pytest.mark.parametrize("q8", [False, True], ids=["hl8", "q8"])
def test_gather_cols_moves_records(dev, hb, q8, Ga, Gb, H):
    """ncols = 2 with col1 = -1 (one strip) and col1 = W - 2 (the call of ssm_amd/subpixel.py): dst rows 0..1 and 3..4 are the source
    columns' 16-byte records of both planes, byte for byte; row 2 and everything else keeps the 0x5a pre-fill.  H around the 256-row
    blocks.  (Q8 with Ga = 1: a record copy does not care that the pair is incomplete.)"""
    lib, B, W, ncols = hb.load(), 2, 7, 2
    g = torch.Generator().manual_seed(H + 10 * Ga + Gb)
    srcs = []
    for G in (Ga, Gb):
        if not G:
            srcs.append(None)
            continue
        p = hb.HPlanes(B, 8 * G, H, W, dev, groups=G)
        n = B * G * 2 * p.Hp * p.Wp * 8
        p.buf[:n] = torch.randint(-30000, 30000, (n,), generator=g, dtype=torch.int16).view(torch.float16).to(dev)     # any bytes
        srcs.append(p)
    pa, pb = srcs
    for col1 in (-1, W - 2):
        dst = hb.HPlanes(B, 8 * (Ga + Gb), 2 * ncols + 1, H, dev, groups=Ga + Gb)
        dst.buf.view(torch.int16).fill_(0x5a5a)
        hb.check(lib.ssm_hl8_gather_cols(pa.view(), Ga, pb.view() if Gb else hb.NULL_HVIEW, Gb, dst.view(), B, H, 0, ncols, col1, hb.stream_ptr()))
        torch.cuda.synchronize()
        got = i16(L.planes(dst))
        want = torch.full_like(got, 0x5a5a)
        src = i16(torch.cat([L.planes(p) for p in srcs if p is not None], 1))          # [B, Ga + Gb, 2, Hp, Wp, 8]
        for r, col in [(0, 0), (1, 1)] + ([(3, col1), (4, col1 + 1)] if col1 >= 0 else []):
            want[:, :, :, L.PADY + r, L.PADX:L.PADX + H] = src[:, :, :, L.PADY:L.PADY + H, L.PADX + col]
        assert torch.equal(got, want), "H=%d col1=%d: %d halves differ" % (H, col1, int((got != want).sum()))
        tail = dst.buf[got.numel():].view(torch.int16)
        assert bool((tail == 0x5a5a).all()), "wrote behind the last plane"
