"""The element-wise and gather kernels every inferred frame passes through (the forward kernels of csrc/ssm_elem.hip), each called through the
C ABI on its own and held to a float64 reference (tests/train_refs.py): the bilinear sampler (ssm_warp_bilinear_fwd), the stage-2 input
builder (ssm_flowinterp_inputs_fwd / _t_fwd), the synthesis (ssm_synthesize_fwd and the one fused into ssm_final_conv_fwd), the 2x2 mean,
concat + bilinear x2, the split-K finish and the strided copy.  The forward twin of tests/test_hip_train_elementwise.py, same yardstick.

Yardstick: err = largest error relative to the largest reference entry (train_refs.rel_err); e_ref = the fp32 CPU oracle's own distance from
the float64 oracle on the same inputs (train_refs.ref_gap), computed at run time.  Assertion: err <= max(8 * e_ref, 4 * 2**-24).
No entry is left out anywhere: a sample is continuous in its coordinate (a tap that floor() assigns differently in fp32 and float64
carries a weight near 0), so the excluded share is 0 and no keep_mask is used.
Exact-arithmetic kernels (2x2 mean, bilinear x2, split-K finish) run on integer-valued inputs, where every product with 1/4, 3/4, 1/8
and every sum is exact in fp32: their outputs must be the float64 reference cast down, bit for bit.  ssm_copy_view: bit equality.

Every call: outputs pre-filled with NaN (or a sentinel where part of the tensor must survive), finite afterwards, the zero frame of padded
planes still zero, and a canary in the tail slack behind the last plane bit-unchanged.  Layouts: contiguous NCHW and padded planes.

Measured on an MI355X (largest figure of each group over all its cases; 830 comparisons in all):
  group            cases  largest err   e_ref there   e_ref range            err / bar
  warp-fwd            14  6.14e-06      6.14e-06      1.7e-07 .. 6.1e-06     0.13
  warp-fwd-grid        4  2.41e-08      2.41e-08      2.3e-08 .. 2.4e-08     0.10
  inputs-fwd          14  4.35e-06      4.35e-06      2.3e-07 .. 4.3e-06     0.13
  inputs-t-ends        2  4.78e-06      4.78e-06      4.8e-06                0.12
  synthesize          28  6.00e-06      6.00e-06      1.3e-07 .. 6.0e-06     0.13
  splitk-finish 0.1   72  7.15e-09      7.15e-09      2.6e-09 .. 7.2e-09     0.03

  In every one of the comparisons err equals e_ref to the four digits printed (largest err / e_ref = 1.00): these kernels are the fp32 CPU
  oracle's arithmetic, step for step, and the suite found no defect in them.  Excluded share: 0 everywhere.

  bit equality (no figure): ssm_flowinterp_inputs_t_fwd against the full kernel, y3 with and without aux, the synthesis fused into
  ssm_final_conv_fwd (both SSM_FINAL_VALU forms) against ssm_final_conv_fwd + ssm_synthesize_fwd, the pass-through channels of the
  stage-2 input, ssm_avgpool2_fwd, ssm_upsample2x_cat_fwd, ssm_splitk_finish_fwd (all options but slope 0.1) and ssm_copy_view.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_refs as R  # noqa: E402
from train_refs import Box, bits, dptr, report  # noqa: E402

pytestmark = pytest.mark.gpu
NAN = float("nan")
SENT = -123.25
F64 = torch.float64
_ids = lambda v: str(v).replace(" ", "")     # noqa: E731


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def hb():
    from ssm_amd import hipbind
    hipbind.load()
    return hipbind


def out_box(hb, dev, layout, shape, fill=NAN):
    """An output: pre-filled, with the canary planted in the slack behind its last plane."""
    return R.plant_canary(Box(hb, dev, layout, shape=shape, fill=fill))


def check_out(box, name):
    """What holds after every call: finite, zero frame, canary unchanged.  Returns the tensor on the CPU."""
    got = box.get()
    assert bool(torch.isfinite(got).all()), "%s: not finite (or not written)" % name
    assert box.frame_is_zero(), "%s: wrote into the zero frame" % name
    assert R.canary_intact(box), "%s: wrote behind the last plane" % name
    return got


def held(name, got, want, e_ref, worst):
    err = R.rel_err(got, want)
    worst[:] = max(worst, [err / R.bar(e_ref), err, e_ref])
    print("  %s: err %.3e e_ref %.3e" % (name, err, e_ref))
    assert err <= R.bar(e_ref), (name, err, e_ref)


# ======================================================================================================================
# samplers
# ======================================================================================================================
@pytest.mark.parametrize("layout", R.LAYOUTS)
@pytest.mark.parametrize("shape,scale", R.SAMPLER_CASES, ids=_ids)
def test_warp_fwd(dev, hb, shape, scale, layout):
    """ssm_warp_bilinear_fwd against O.warp in float64, C in {1, 3, 6}; (2, 1, 5) and (1, 37, 1) have an axis of one pixel (the
    max(size - 1, 1) normalisation: the coordinate is 0 whatever the flow)."""
    lib, st = hb.load(), hb.stream_ptr
    B, H, W = shape
    worst = [0.0, 0.0, 0.0]
    for C in (1, 3, 6):
        g = torch.Generator().manual_seed(R.SEED + C)
        img = torch.randn(B, C, H, W, generator=g)
        flow = torch.randn(B, 2, H, W, generator=g) * scale
        want = R.warp_fwd(img, flow, F64)
        e_ref = R.ref_gap(lambda dt: R.warp_fwd(img, flow, dt))
        bi, bf, out = Box(hb, dev, layout, img), Box(hb, dev, layout, flow), out_box(hb, dev, layout, (B, C, H, W))
        hb.check(lib.ssm_warp_bilinear_fwd(bi.view(), bf.view(), out.view(), B, C, H, W, st()))
        held("C=%d" % C, check_out(out, "out"), want, e_ref, worst)
    report("warp-fwd", "%s x%g %s" % (shape, scale, layout), worst[1], worst[2])


@pytest.mark.parametrize("layout", R.LAYOUTS)
@pytest.mark.parametrize("shape", R.CONSTRUCTED_SHAPES, ids=_ids)
def test_warp_fwd_on_constructed_positions(dev, hb, shape, layout):
    """train_refs.constructed_flow: every sampling position is exactly an integer, exactly W - 1 / H - 1 (the upper tap outside with weight
    0), inside (-1, 0) or (W - 1, W) (taps outside), or at / beyond -1 and W (no tap inside, or inside with weight 0) - all 16 combinations
    of the two axes.  Where an axis is of the last kind the output is exactly zero."""
    lib, st = hb.load(), hb.stream_ptr
    B, H, W = shape
    flow, tx, ty, cx, cy = R.constructed_flow(shape)
    ix, iy = R.sampling_positions(flow)
    assert torch.equal(ix, tx) and torch.equal(iy, ty)          # (tests/test_train_refs_cpu.py holds the family to its classes)
    none_inside = ((cx == 3) | (cy == 3)).unsqueeze(1)
    worst = [0.0, 0.0, 0.0]
    for C in (1, 3, 6):
        g = torch.Generator().manual_seed(R.SEED + C)
        img = torch.randn(B, C, H, W, generator=g)
        want = R.warp_fwd(img, flow, F64)
        e_ref = R.ref_gap(lambda dt: R.warp_fwd(img, flow, dt))
        bi, bf, out = Box(hb, dev, layout, img), Box(hb, dev, layout, flow), out_box(hb, dev, layout, (B, C, H, W))
        hb.check(lib.ssm_warp_bilinear_fwd(bi.view(), bf.view(), out.view(), B, C, H, W, st()))
        got = check_out(out, "out")
        held("C=%d" % C, got, want, e_ref, worst)
        m = none_inside.expand_as(got)
        assert bool(m.any()) and not bool(got[m].any()), "a sample with no tap inside the image is not exactly zero"
        assert not bool(want[m].any())
    report("warp-fwd-grid", "%s %s" % (shape, layout), worst[1], worst[2])


def _inputs_call(hb, dev, layout, c, fn, out):
    B, _, H, W = c["img6"].shape
    img6, flow4 = Box(hb, dev, layout, c["img6"]), Box(hb, dev, layout, c["flow4"])
    td = c["t"].to(dev)
    hb.check(fn(img6.view(), flow4.view(), dptr(td), out, B, H, W, hb.stream_ptr()))


def _check_inputs(c, got, worst):
    want = R.inputs_fwd(c["img6"], c["flow4"], c["t"], F64)
    lo = R.inputs_fwd(c["img6"], c["flow4"], c["t"], torch.float32)
    for name, a, b in R.INPUT_GROUPS:
        held(name, got[:, a:b], want[:, a:b], R.rel_err(lo[:, a:b], want[:, a:b]), worst)
    # channels 0:3 and 13:16 are copies of the second and the first frame
    assert torch.equal(bits(got[:, 0:3]), bits(c["img6"][:, 3:6])) and torch.equal(bits(got[:, 13:16]), bits(c["img6"][:, 0:3]))


@pytest.mark.parametrize("layout", R.LAYOUTS)
@pytest.mark.parametrize("shape,scale", R.SAMPLER_CASES, ids=_ids)
def test_flowinterp_inputs_fwd(dev, hb, shape, scale, layout):
    """ssm_flowinterp_inputs_fwd: all 16 channels against O.flow_interp_inputs in float64, each channel group (frame copies, warped frames,
    approximated flows) against its own largest entry and its own e_ref; the frame copies bit for bit."""
    lib = hb.load()
    B, H, W = shape
    c = R.make_case(shape, scale)
    out = out_box(hb, dev, layout, (B, 16, H, W))
    _inputs_call(hb, dev, layout, c, lib.ssm_flowinterp_inputs_fwd, out.view())
    worst = [0.0, 0.0, 0.0]
    _check_inputs(c, check_out(out, "out16"), worst)
    report("inputs-fwd", "%s x%g %s" % (shape, scale, layout), worst[1], worst[2])


@pytest.mark.parametrize("layout", R.LAYOUTS)
def test_flowinterp_inputs_at_the_ends_of_the_interval(dev, hb, layout):
    """t = 0 and t = 1 per sample: the coefficient products (1 - t) t, t^2, (1 - t)^2 vanish or are 1, one approximated flow is +-0 and the
    other a copy of a stage-1 flow; channels 6:10 (and the warps by them) equal the reference's to the bar."""
    lib = hb.load()
    shape, scale = (3, 9, 70), 3.0
    B, H, W = shape
    c = R.make_case(shape, scale)
    c["t"] = torch.tensor([0.0, 1.0, 0.0])
    out = out_box(hb, dev, layout, (B, 16, H, W))
    _inputs_call(hb, dev, layout, c, lib.ssm_flowinterp_inputs_fwd, out.view())
    worst = [0.0, 0.0, 0.0]
    got = check_out(out, "out16")
    _check_inputs(c, got, worst)
    assert not bool(got[0, 8:10].any()) and not bool(got[1, 6:8].any())          # t = 0: Ft0^ = 0;  t = 1: Ft1^ = 0
    report("inputs-t-ends", "%s x%g %s" % (shape, scale, layout), worst[1], worst[2])


@pytest.mark.parametrize("layout", R.LAYOUTS)
@pytest.mark.parametrize("shape,scale", R.SAMPLER_CASES, ids=_ids)
def test_flowinterp_inputs_t_fwd(dev, hb, shape, scale, layout):
    """ssm_flowinterp_inputs_t_fwd writes channels 3:13 with the full kernel's bits and nothing else.  out16 is a view at a batch and a
    channel offset into a larger sentinel-filled tensor (the hoisted plan passes in16.view(b0=...) of the stage-2 batch,
    ssm_amd/engine.py run_stage2): the frame channels of the view, the channels either side of it and the batch entry in front of it
    keep the sentinel."""
    lib = hb.load()
    B, H, W = shape
    c = R.make_case(shape, scale)
    full = out_box(hb, dev, layout, (B, 16, H, W))
    _inputs_call(hb, dev, layout, c, lib.ssm_flowinterp_inputs_fwd, full.view())
    want = check_out(full, "out16")
    big = out_box(hb, dev, layout, (B + 1, 18, H, W), fill=SENT)
    _inputs_call(hb, dev, layout, c, lib.ssm_flowinterp_inputs_t_fwd, big.view(c0=1, b0=1))
    got = check_out(big, "out16 (t)")
    assert torch.equal(bits(got[1:, 4:14]), bits(want[:, 3:13])), "channels 3:13 differ from the full kernel's"
    got[1:, 4:14] = SENT
    assert bool((got == SENT).all()), "wrote outside channels 3:13"
    report("inputs-t-bits", "%s x%g %s" % (shape, scale, layout), R.rel_err(big.get()[1:, 4:14], want[:, 3:13]), 0.0)


@pytest.mark.parametrize("saturated", [False, True], ids=["randn1.5", "saturated"])
@pytest.mark.parametrize("layout", R.LAYOUTS)
@pytest.mark.parametrize("shape,scale", R.SAMPLER_CASES, ids=_ids)
def test_synthesize_fwd(dev, hb, shape, scale, layout, saturated):
    """ssm_synthesize_fwd: y3 against O.synthesize and aux (Ft1 | Ft0 | V0) against in16[:, 6:10] + out5[:, 1:5] and 1 - sigmoid(out5[:, 0])
    in float64; aux NULL and given (y3 bit-identical).  saturated: the visibility logit times 40, so expf overflows to inf where it is
    negative (V1 = 0) and V1 rounds to 1 where it is positive (V0 = 0); t inside (0, 1) keeps the denominator >= 0.125."""
    lib, st = hb.load(), hb.stream_ptr
    B, H, W = shape
    c = R.saturated_case(shape, scale) if saturated else R.make_case(shape, scale)
    in16 = R.inputs_fwd(c["img6"], c["flow4"], c["t"], F64).float()          # an fp32 input like the others, from the reference
    want = R.synth_fwd(c["img6"], in16, c["out5"], c["t"], F64)
    lo = R.synth_fwd(c["img6"], in16, c["out5"], c["t"], torch.float32)
    assert all(bool(torch.isfinite(z).all()) for z in lo), "the fp32 oracle is not finite on this case"
    img6, b16, out5 = (Box(hb, dev, layout, x) for x in (c["img6"], in16, c["out5"]))
    td = c["t"].to(dev)
    y3a, y3b, aux = (out_box(hb, dev, layout, (B, n, H, W)) for n in (3, 3, 5))
    hb.check(lib.ssm_synthesize_fwd(img6.view(), b16.view(), out5.view(), dptr(td), y3a.view(), hb.NULL_VIEW, B, H, W, st()))
    hb.check(lib.ssm_synthesize_fwd(img6.view(), b16.view(), out5.view(), dptr(td), y3b.view(), aux.view(), B, H, W, st()))
    ga, gb, gx = check_out(y3a, "y3"), check_out(y3b, "y3 (aux given)"), check_out(aux, "aux")
    assert torch.equal(bits(ga), bits(gb)), "y3 depends on whether aux is asked for"
    worst = [0.0, 0.0, 0.0]
    for name, got, w, l in (("y3", ga, want[0], lo[0]), ("aux flows", gx[:, 0:4], want[1], lo[1]), ("aux V0", gx[:, 4:5], want[2], lo[2])):
        held(name, got, w, R.rel_err(l, w), worst)
    if saturated:
        v0 = gx[:, 4]
        assert bool((v0 == 0).any()) and bool((v0 == 1).any()), "the case does not saturate"
    report("synthesize", "%s x%g %s %s" % (shape, scale, layout, "sat" if saturated else ""), worst[1], worst[2])


@pytest.mark.parametrize("form", ["1", "0"], ids=["valu", "mfma4x4"])
@pytest.mark.parametrize("layout", R.LAYOUTS)
@pytest.mark.parametrize("shape,scale", [((1, 5, 65), 2.0), ((3, 9, 70), 3.0)], ids=_ids)
def test_final_conv_fused_synthesis_is_the_two_kernel_path_bit_for_bit(dev, hb, shape, scale, layout, form, monkeypatch):
    """ssm_final_conv_fwd writing out5, then ssm_synthesize_fwd on that out5, give the y3 and the aux of the fused call bit for bit (both
    run synth_pixel on the same five sums), for both forms of the convolution; the fused call with and without the 5-channel map."""
    monkeypatch.setenv("SSM_FINAL_VALU", form)
    lib, st = hb.load(), hb.stream_ptr
    B, H, W = shape
    c = R.make_case(shape, scale)
    g = torch.Generator().manual_seed(77)
    x = torch.randn(B, 32, H, W, generator=g)
    w = (torch.randn(5, 32, 3, 3, generator=g) / (32 * 9) ** 0.5 * 3.0).to(dev)     # residual flows of a few px, logits of a few units
    bias = (torch.randn(5, generator=g) * 0.1).to(dev)
    in16 = R.inputs_fwd(c["img6"], c["flow4"], c["t"], F64).float()
    px = hb.Planes(B, 32, H, W, dev).load(x.to(dev))
    img6, b16 = Box(hb, dev, layout, c["img6"]), Box(hb, dev, layout, in16)
    td, nv = c["t"].to(dev), hb.NULL_VIEW
    new = lambda n: out_box(hb, dev, layout, (B, n, H, W))     # noqa: E731
    o5, y3s, auxs = new(5), new(3), new(5)
    hb.check(lib.ssm_final_conv_fwd(px.view(), dptr(w), dptr(bias), 5, o5.view(), nv, nv, None, nv, nv, B, H, W, st()))
    hb.check(lib.ssm_synthesize_fwd(img6.view(), b16.view(), o5.view(), dptr(td), y3s.view(), auxs.view(), B, H, W, st()))
    ref = [check_out(z, n) for z, n in ((o5, "out5"), (y3s, "y3"), (auxs, "aux"))]
    y3f, auxf = new(3), new(5)          # the plan's call: the 5-channel map is not written
    hb.check(lib.ssm_final_conv_fwd(px.view(), dptr(w), dptr(bias), 5, nv, img6.view(), b16.view(), dptr(td), y3f.view(), auxf.view(), B, H, W,
                                    st()))
    o5g, y3g, auxg = new(5), new(3), new(5)          # ... and with it (the training step reads it)
    hb.check(lib.ssm_final_conv_fwd(px.view(), dptr(w), dptr(bias), 5, o5g.view(), img6.view(), b16.view(), dptr(td), y3g.view(), auxg.view(),
                                    B, H, W, st()))
    for name, box, want in (("y3 fused", y3f, ref[1]), ("aux fused", auxf, ref[2]), ("out5 fused", o5g, ref[0]), ("y3 fused+out5", y3g, ref[1]),
                            ("aux fused+out5", auxg, ref[2])):
        assert torch.equal(bits(check_out(box, name)), bits(want)), name
    report("final-synth", "%s %s form=%s" % (shape, layout, form), R.rel_err(y3f.get(), ref[1]), 0.0)


# ======================================================================================================================
# exact-arithmetic kernels: integer-valued inputs, bit equality with the float64 reference cast down
# ======================================================================================================================
@pytest.mark.parametrize("layout", R.LAYOUTS)
@pytest.mark.parametrize("H,W", R.AVGPOOL_HW, ids=_ids)
@pytest.mark.parametrize("C", R.AVGPOOL_C)
def test_avgpool2_fwd_exact(dev, hb, C, H, W, layout):
    """ssm_avgpool2_fwd: C covers the split of the channels into groups of 4 (ragged, whole, several + 1)."""
    from oracle import ssm_oracle as O
    lib, st = hb.load(), hb.stream_ptr
    x = R.avgpool_case(C, H, W)
    B = x.shape[0]
    want = R.exact_f32(O.avg_pool2(x.double()))
    bx, out = Box(hb, dev, layout, x), out_box(hb, dev, layout, (B, C, H // 2, W // 2))
    hb.check(lib.ssm_avgpool2_fwd(bx.view(), out.view(), B, C, H, W, st()))
    got = check_out(out, "y")
    report("avgpool2", "C=%d %dx%d %s" % (C, H, W, layout), R.rel_err(got, want), 0.0)
    assert torch.equal(bits(got), bits(want))


@pytest.mark.parametrize("layout", R.LAYOUTS)
@pytest.mark.parametrize("h,w", R.UPSAMPLE_HW, ids=_ids)
@pytest.mark.parametrize("Ca,Cb", R.UPSAMPLE_CH, ids=_ids)
def test_upsample2x_cat_fwd_exact(dev, hb, Ca, Cb, h, w, layout):
    """ssm_upsample2x_cat_fwd against O.upsample2x_bilinear(cat) in float64.  Planes take the 16-byte stores, NCHW outputs whose width is no
    multiple of 4 the element stores; odd w: the last thread of a row owns one source pixel; (8, 8) on (5, 7): the second source is
    batch-broadcast (sb = 0), as conv7a's cross-skip source is."""
    from oracle import ssm_oracle as O
    lib, st = hb.load(), hb.stream_ptr
    bcast = (Ca, Cb, h, w) == (8, 8, 5, 7)
    a, b, cat = R.upsample_case(Ca, Cb, h, w, bcast=bcast)
    B = a.shape[0]
    want = R.exact_f32(O.upsample2x_bilinear(cat.double()))
    ba, bb = Box(hb, dev, layout, a), (Box(hb, dev, layout, b) if Cb else None)
    vb = bb.view() if Cb else hb.NULL_VIEW
    if bcast:
        vb.sb = 0
    out = out_box(hb, dev, layout, (B, Ca + Cb, 2 * h, 2 * w))
    hb.check(lib.ssm_upsample2x_cat_fwd(ba.view(), Ca, vb, Cb, out.view(), B, h, w, st()))
    got = check_out(out, "y")
    report("upsample2x", "Ca=%d Cb=%d %dx%d %s%s" % (Ca, Cb, h, w, layout, " bcast" if bcast else ""), R.rel_err(got, want), 0.0)
    assert torch.equal(bits(got), bits(want))


@pytest.mark.parametrize("layout", R.LAYOUTS)
@pytest.mark.parametrize("H,W", R.FINISH_HW, ids=_ids)
@pytest.mark.parametrize("C", R.FINISH_C)
@pytest.mark.parametrize("KS", R.FINISH_KS)
def test_splitk_finish_fwd_exact(dev, hb, KS, C, H, W, layout):
    """ssm_splitk_finish_fwd by its header contract (include/ssm_hip.h): y = act(sum_ks part[ks * B + b] + add[b / add_div]), SSM_FLAG_MASK:
    y = sum * (add > 0 ? 1 : slope); pool = the 2x2 mean of y.  "bias only" is the plain sum (the bias arrives inside partial 0).  Slope
    0.125 is passed explicitly, so every option is exact on integer-valued planes: bit equality with the float64 formula.  One option
    cannot be exact - the model's slope 0.1: it is held to bar(e_ref), e_ref = the same formula in fp32 on the CPU against float64.
    The fused mean runs where H and W are even; (11, 11) takes the one-pixel kernel, (5, 6) has a lone last row."""
    lib, st = hb.load(), hb.stream_ptr
    d = R.finish_case(KS, C, H, W)
    B = d["part"].shape[0] // KS
    part = Box(hb, dev, layout, d["part"])
    adds = {n: Box(hb, dev, layout, d[n]) for n in (1, 2)}
    ran = 0
    for name, div, lrelu, mask, pool, slope in R.FINISH_OPTIONS:
        if pool and (H % 2 or W % 2):
            continue
        kw = dict(add=d[div] if div else None, add_div=max(div, 1), slope=slope, lrelu=lrelu, mask=mask, pool=pool)
        wy, wp = R.splitk_finish_ref(d["part"], KS, dtype=F64, **kw)
        y, yp = out_box(hb, dev, layout, (B, C, H, W)), (out_box(hb, dev, layout, (B, C, H // 2, W // 2)) if pool else None)
        flags = hb.SSM_FLAG_MASK if mask else (hb.SSM_FLAG_LRELU if lrelu else 0)
        hb.check(lib.ssm_splitk_finish_fwd(part.view(), KS, y.view(), yp.view() if pool else hb.NULL_VIEW,
                                           adds[div].view() if div else hb.NULL_VIEW, max(div, 1), B, C, H, W, slope, flags, st()))
        got, gp = check_out(y, name), (check_out(yp, name + " pool") if pool else None)
        if slope == R.FINISH_SLOPE:
            assert torch.equal(bits(got), bits(R.exact_f32(wy))), name
            if pool:
                assert torch.equal(bits(gp), bits(R.exact_f32(wp))), name + " pool"
            err, e_ref = R.rel_err(got, wy), 0.0
        else:
            err, e_ref = R.rel_err(got, wy), R.rel_err(R.splitk_finish_ref(d["part"], KS, dtype=torch.float32, **kw)[0], wy)
            assert err <= R.bar(e_ref), (name, err, e_ref)
        print("  %s: err %.3e e_ref %.3e" % (name, err, e_ref))
        ran += 1
    report("splitk-finish", "KS=%d C=%d %dx%d %s (%d options)" % (KS, C, H, W, layout, ran), err, e_ref)


def _special(shape, seed):
    """randn with +0, -0, the smallest subnormal, inf and a large value planted: a copy moves bits."""
    x = torch.randn(shape, generator=torch.Generator().manual_seed(seed))
    flat = x.view(-1)
    for i, v in enumerate((0.0, -0.0, 2.0 ** -149, float("inf"), -3.0e38)):
        flat[i::11] = v
    return x


def test_copy_view_bit_exact(dev, hb):
    """ssm_copy_view: NCHW -> planes, planes -> NCHW, planes -> planes at a channel offset and at view(y0=, x0=) origins on both sides, and a
    batch-broadcast source.  The destination is larger than the block and pre-filled with a sentinel: the block arrives bit for bit, the
    neighbouring channels, rows and columns keep the sentinel, the zero frame stays zero and the tail canary unchanged."""
    lib, st = hb.load(), hb.stream_ptr
    B, C, H, W = 2, 3, 5, 65
    x = _special((B, C, H, W), 5)

    def expect(shape, c0, y0, x0, block):
        e = torch.full(shape, SENT)
        e[:block.shape[0], c0:c0 + block.shape[1], y0:y0 + block.shape[2], x0:x0 + block.shape[3]] = block
        return e

    def finish(dst, want, case):
        assert dst.frame_is_zero() and R.canary_intact(dst), case
        assert torch.equal(bits(dst.get()), bits(want)), case
        report("copy-view", case, 0.0, 0.0)

    # NCHW -> planes at channel 1 of 5
    src, dst = Box(hb, dev, "nchw", x), out_box(hb, dev, "planes", (B, 5, H, W), fill=SENT)
    hb.check(lib.ssm_copy_view(src.view(), dst.view(c0=1), B, C, H, W, st()))
    finish(dst, expect((B, 5, H, W), 1, 0, 0, x), "nchw -> planes c0=1")
    # planes -> NCHW at channel 1 of 5
    src, dst = Box(hb, dev, "planes", x), out_box(hb, dev, "nchw", (B, 5, H, W), fill=SENT)
    hb.check(lib.ssm_copy_view(src.view(), dst.view(c0=1), B, C, H, W, st()))
    finish(dst, expect((B, 5, H, W), 1, 0, 0, x), "planes -> nchw c0=1")
    # planes -> planes: source origin (1, 2) of a larger map, destination channel 2, origin (2, 3) of a larger map
    big = _special((B, C, H + 3, W + 4), 6)
    src, dst = Box(hb, dev, "planes", big), out_box(hb, dev, "planes", (B, 6, H + 4, W + 5), fill=SENT)
    hb.check(lib.ssm_copy_view(src.p.view(y0=1, x0=2), dst.p.view(c0=2, y0=2, x0=3), B, C, H, W, st()))
    finish(dst, expect((B, 6, H + 4, W + 5), 2, 2, 3, big[:, :, 1:1 + H, 2:2 + W]), "planes(y0=1,x0=2) -> planes(c0=2,y0=2,x0=3)")
    # batch-broadcast source (sb = 0) -> three entries, from both layouts
    for layout in R.LAYOUTS:
        src, dst = Box(hb, dev, layout, x[:1]), out_box(hb, dev, "planes", (3, 4, H, W), fill=SENT)
        v = src.view()
        v.sb = 0
        hb.check(lib.ssm_copy_view(v, dst.view(c0=1), 3, C, H, W, st()))
        finish(dst, expect((3, 4, H, W), 1, 0, 0, x[:1].expand(3, -1, -1, -1)), "%s broadcast -> planes c0=1" % layout)
