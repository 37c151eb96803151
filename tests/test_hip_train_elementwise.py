"""The non-convolution kernels of a training step (csrc/ssm_bwd.hip, csrc/ssm_rnn.hip), each called through the C ABI on its own and held
to a float64 reference (tests/train_refs.py): loss reductions, bilinear-sampler adjoints, activation / pool / upsample adjoints, the bias
reduction, the recurrent cells and their adjoints.

Yardstick: err = largest error over the kept entries relative to the largest reference entry (bias: relative to sum |dz| of the channel);
e_ref = the fp32 CPU oracle's own distance from the float64 oracle on the same inputs (train_refs.ref_gap), computed at run time.
Assertion: err <= max(8 * e_ref, 4 * 2**-24), or bit equality where the operation is a fixed sequence of single fp32 operations.
Kept pixels (sampler adjoints only): train_refs.keep_mask - at most 1 % may be dropped, asserted in every case.

Measured on an MI355X (largest figure of each group over all its cases; excluded = largest share keep_mask dropped in a case):
  group            cases  largest err   e_ref there   e_ref range            err / bar
  sampler-adjoint     14  3.46e-06      3.40e-06      6.6e-08 .. 3.4e-06     0.26
  warp-adjoint        14  2.64e-06      2.61e-06      6.6e-08 .. 2.6e-06     0.16
  loss-sums           18  2.69e-07      1.01e-07      1.6e-08 .. 1.2e-07     0.94
  sqdiff-mean          8  2.16e-07      9.55e-08      8.8e-09 .. 9.6e-08     0.90
  sqdiff-grad          8  8.71e-08      8.71e-08      3.7e-08 .. 8.7e-08     0.13
  bias-grad           12  6.34e-08      6.34e-08      2.6e-10 .. 6.3e-08     0.14
  upsample-adj        12  1.47e-07      1.47e-07      7.8e-08 .. 1.9e-07     0.16
  lstm-cell           24  2.01e-07      1.43e-07      3.7e-08 .. 1.8e-07     0.27
  gru-cell            24  1.36e-06      1.36e-06      5.4e-08 .. 1.4e-06     0.21

  excluded sampler-adjoint  (2, 20, 28) x2         0.089 %
  excluded sampler-adjoint  (3, 9, 70) x3          0.106 %
  excluded sampler-adjoint  (1, 4, 64) x2          0.000 %
  excluded sampler-adjoint  (1, 5, 65) x2          0.308 %
  excluded sampler-adjoint  (2, 1, 5) x1           0.000 %
  excluded sampler-adjoint  (1, 37, 1) x1          0.000 %
  excluded sampler-adjoint  (2, 5, 3) x6           0.000 %
  excluded warp-adjoint     (2, 20, 28) x2         0.000 %
  excluded warp-adjoint     (3, 9, 70) x3          0.000 %
  excluded warp-adjoint     (1, 4, 64) x2          0.391 %
  excluded warp-adjoint     (1, 5, 65) x2          0.308 %
  excluded warp-adjoint     (2, 1, 5) x1           0.000 %
  excluded warp-adjoint     (1, 37, 1) x1          0.000 %
  excluded warp-adjoint     (2, 5, 3) x6           0.000 %

  bit equality (no figure): ssm_lrelu_bwd on every path, ssm_lrelu_bwd_q8's fp32 twin, the mask form of the upsample adjoint, the
  one-pixel against the two-pixel upsample kernel, ssm_maxpool2_fwd / _bwd against torch, repeated loss-sum / sqdiff-mean calls.
  The loss sums and the sqdiff mean sit closest to their bar: 64 chunk sums are added one after the other in fp32.
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
TERMS = [(1, 1), (0, 1), (1, 0), (0, 0)]
LAYOUTS = ["contiguous", "planes"]
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


# ======================================================================================================================
# sampler adjoints
# ======================================================================================================================
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape,scale", R.SAMPLER_CASES, ids=_ids)
def test_synthesis_and_inputs_adjoints(dev, hb, shape, scale, layout):
    """ssm_synthesize_bwd + ssm_flowinterp_inputs_bwd against float64 autograd: the four (stage1_terms, stage2_terms) combinations, dy_extra
    NULL and given, contiguous tensors and padded planes (est4 = the channel-offset view in16.view(6) the planned step passes).
    Regression cases: (2, 1, 5) and (1, 37, 1).  On an axis of one pixel the reference's sampling coordinate is 0 * (...), so the
    sample does not depend on that flow component; the kernels took d ix / d u = 1 there and returned gradients 55-75 % of the
    largest entry off (sample_d in csrc/ssm_bwd.hip now scales by (W - 1) / max(W - 1, 1))."""
    lib, st = hb.load(), hb.stream_ptr
    B, H, W = shape
    c = R.make_case(shape, scale)
    mk = lambda x: Box(hb, dev, layout, x)     # noqa: E731
    img6, flow4, out5, tgt, r16, dyx = (mk(c[k]) for k in ("img6", "flow4", "out5", "target", "r16", "dy_extra"))
    td, crd, cwd = c["t"].to(dev), c["c_rec"].to(dev), c["c_warp"].to(dev)
    worst, top_share = [0.0, 0.0, 0.0], 0.0
    for s1, s2 in TERMS:
        for extra in (None, c["dy_extra"]):
            args = (c["img6"], c["flow4"], c["out5"], c["target"], c["t"], c["c_rec"], c["c_warp"], c["r16"], extra, s1, s2)
            ref = R.loss_and_grads(*args, dtype=torch.float64)
            lo = R.loss_and_grads(*args, dtype=torch.float32)
            keep = R.keep_mask(ref["flows"], ref["l1_args"])
            share = R.excluded_share(keep)
            top_share = max(top_share, share)
            assert share <= 0.01, share
            in16 = mk(ref["in16"].float())
            dout5, dest, dflow4 = (Box(hb, dev, layout, shape=(B, n, H, W)) for n in (5, 4, 4))
            hb.check(lib.ssm_synthesize_bwd(img6.view(), in16.view(6), out5.view(), tgt.view(), dptr(td), dptr(crd), dptr(cwd),
                                            dyx.view() if extra is not None else hb.NULL_VIEW, dout5.view(), dest.view(), B, H, W, s2, st()))
            hb.check(lib.ssm_flowinterp_inputs_bwd(img6.view(), flow4.view(), r16.view(), dest.view(), dptr(td), dptr(cwd), dflow4.view(),
                                                   B, H, W, s1, st()))
            for name, got in (("dout5", dout5), ("dflow4", dflow4)):
                g = got.get()
                assert bool(torch.isfinite(g).all()) and got.frame_is_zero(), name
                err, e_ref = R.rel_err(g, ref[name], keep), R.rel_err(lo[name], ref[name], keep)
                worst = max(worst, [err / R.bar(e_ref), err, e_ref])
                print("  terms (%d,%d) extra %d %s: err %.3e e_ref %.3e excluded %.3f %%" % (s1, s2, extra is not None, name, err, e_ref, 100 * share))
                assert err <= R.bar(e_ref), (name, s1, s2, extra is not None, err, e_ref)
            # the gradient wrt the approximated flows equals the one wrt the refinements (Ft = Ft^ + dFt)
            assert torch.equal(dest.get(), dout5.get()[:, 1:5])
    report("sampler-adjoint", "%s x%g %s" % (shape, scale, layout), worst[1], worst[2], top_share)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape,scale", R.SAMPLER_CASES, ids=_ids)
def test_warp_adjoint(dev, hb, shape, scale, layout):
    """ssm_warp_bilinear_bwd called directly: C in {1, 3, 6}; dflow only, dimg only, both; a second call into the same dimg doubles it."""
    lib, st = hb.load(), hb.stream_ptr
    B, H, W = shape
    worst = [0.0, 0.0, 0.0]
    for C in (1, 3, 6):
        g = torch.Generator().manual_seed(R.SEED + C)
        img, dy = torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g)
        flow = torch.randn(B, 2, H, W, generator=g) * scale
        keep = R.keep_mask([flow])
        share = R.excluded_share(keep)
        assert share <= 0.01, share
        want = R.warp_grads(img, flow, dy, torch.float64)
        lo = R.warp_grads(img, flow, dy, torch.float32)
        e_flow, e_img = R.rel_err(lo[0], want[0], keep), R.rel_err(lo[1], want[1])
        bi, bf, bd = (Box(hb, dev, layout, x) for x in (img, flow, dy))
        for want_flow, want_img in ((1, 0), (0, 1), (1, 1)):
            dflow = Box(hb, dev, layout, shape=(B, 2, H, W))
            dimg = Box(hb, dev, layout, shape=(B, C, H, W), fill=0.0)
            call = lambda: hb.check(lib.ssm_warp_bilinear_bwd(bi.view(), bf.view(), bd.view(), dflow.view() if want_flow else hb.NULL_VIEW,     # noqa: E731
                                                              dimg.view() if want_img else hb.NULL_VIEW, B, C, H, W, st()))
            call()
            if want_flow:
                err = R.rel_err(dflow.get(), want[0], keep)
                worst = max(worst, [err / R.bar(e_flow), err, e_flow])
                assert err <= R.bar(e_flow), ("dflow", C, err, e_flow)
                assert dflow.frame_is_zero()
            else:
                assert bool(torch.isnan(dflow.get()).all())          # not asked for: not written
            if want_img:
                err = R.rel_err(dimg.get(), want[1])
                worst = max(worst, [err / R.bar(e_img), err, e_img])
                assert err <= R.bar(e_img), ("dimg", C, err, e_img)
                call()                                                  # accumulates: twice the gradient
                err = R.rel_err(dimg.get(), 2 * want[1])
                assert err <= R.bar(e_img), ("dimg x2", C, err, e_img)
                assert dimg.frame_is_zero()
            else:
                assert not bool(dimg.get().any())
    report("warp-adjoint", "%s x%g %s" % (shape, scale, layout), worst[1], worst[2], share)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_samplers_with_every_tap_outside_give_exact_zeros(dev, hb, layout):
    """All flows at 1e6: no tap lands in the image, so dflow and dimg are exactly zero (and nothing is NaN or out of range)."""
    lib, st = hb.load(), hb.stream_ptr
    B, C, H, W = 2, 3, 5, 66
    g = torch.Generator().manual_seed(R.SEED)
    img, dy = torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g)
    for val in (1e6, -1e6):
        bi, bf, bd = Box(hb, dev, layout, img), Box(hb, dev, layout, torch.full((B, 2, H, W), val)), Box(hb, dev, layout, dy)
        dflow, dimg = Box(hb, dev, layout, shape=(B, 2, H, W)), Box(hb, dev, layout, shape=(B, C, H, W), fill=0.0)
        hb.check(lib.ssm_warp_bilinear_bwd(bi.view(), bf.view(), bd.view(), dflow.view(), dimg.view(), B, C, H, W, st()))
        assert not bool(dflow.get().any()) and not bool(dimg.get().any())
        assert dimg.frame_is_zero() and dflow.frame_is_zero()
    # the fused adjoints: flows of 1e6 through est4 (synthesis) and flow4 (inputs, all four terms on)
    c = R.make_case((B, H, W), 1.0)
    mk = lambda x: Box(hb, dev, layout, x)     # noqa: E731
    img6, out5, tgt, r16 = mk(c["img6"]), mk(c["out5"]), mk(c["target"]), mk(torch.zeros(B, 16, H, W))
    in16, flow4 = mk(torch.full((B, 16, H, W), 1e6)), mk(torch.full((B, 4, H, W), 1e6))
    td, crd, cwd = c["t"].to(dev), c["c_rec"].to(dev), c["c_warp"].to(dev)
    dout5, dest, dflow4 = (Box(hb, dev, layout, shape=(B, n, H, W)) for n in (5, 4, 4))
    hb.check(lib.ssm_synthesize_bwd(img6.view(), in16.view(6), out5.view(), tgt.view(), dptr(td), dptr(crd), dptr(cwd), hb.NULL_VIEW,
                                    dout5.view(), dest.view(), B, H, W, 1, st()))
    assert not bool(dest.get().any()) and not bool(dout5.get()[:, 1:5].any()) and bool(torch.isfinite(dout5.get()).all())
    hb.check(lib.ssm_flowinterp_inputs_bwd(img6.view(), flow4.view(), r16.view(), dest.view(), dptr(td), dptr(cwd), dflow4.view(), B, H, W, 1,
                                           st()))
    assert not bool(dflow4.get().any())


# ======================================================================================================================
# loss reductions
# ======================================================================================================================
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape,scale", R.SAMPLER_CASES + R.LOSS_ONLY_CASES, ids=_ids)
def test_train_loss_sums(dev, hb, shape, scale, layout):
    """ssm_train_loss_sums: both per-sample sums against float64 under the four flag combinations (unmasked: the sums are continuous);
    NaN in the scratch buffer must not reach the result, `out` is a slice of a larger buffer whose other entries survive, and a second
    call returns the same bits."""
    lib, st = hb.load(), hb.stream_ptr
    B, H, W = shape
    c = R.make_case(shape, scale)
    mk = lambda x: Box(hb, dev, layout, x)     # noqa: E731
    img6, flow4, out5, tgt = (mk(c[k]) for k in ("img6", "flow4", "out5", "target"))
    worst = [0.0, 0.0, 0.0]
    for s1, s2 in TERMS:
        args = (c["img6"], c["flow4"], c["out5"], c["target"], c["t"], c["c_rec"], c["c_warp"], None, None, s1, s2)
        ref, lo = R.loss_and_grads(*args, dtype=torch.float64), R.loss_and_grads(*args, dtype=torch.float32)
        in16, pred = mk(ref["in16"].float()), mk(ref["pred"].float())
        outs = []
        for _ in range(2):
            scratch = torch.full((128 * B,), NAN, device=dev)
            buf = torch.full((2 * B + 8,), -7.5, device=dev)
            out = buf[4:4 + 2 * B]
            hb.check(lib.ssm_train_loss_sums(img6.view(), flow4.view(), in16.view(6), out5.view(), pred.view(), tgt.view(), dptr(scratch),
                                             dptr(out), B, H, W, s1, s2, st()))
            b = buf.cpu()
            assert bool((b[:4] == -7.5).all()) and bool((b[4 + 2 * B:] == -7.5).all()), "wrote outside out[2B]"
            outs.append(b[4:4 + 2 * B].view(B, 2))
        assert bool(torch.isfinite(outs[0]).all())
        assert torch.equal(bits(outs[0]), bits(outs[1])), "two calls differ"
        err, e_ref = R.rel_err(outs[0], ref["sums"]), R.rel_err(lo["sums"], ref["sums"])
        worst = max(worst, [err / R.bar(e_ref), err, e_ref])
        print("  terms (%d,%d): err %.3e e_ref %.3e" % (s1, s2, err, e_ref))
        assert err <= R.bar(e_ref), (s1, s2, err, e_ref)
        if not s1 and not s2:
            assert not bool(outs[0][:, 1].any())
    report("loss-sums", "%s x%g %s" % (shape, scale, layout), worst[1], worst[2])


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("chw", [(7, 1, 1), (1, 8, 8), (10, 12, 20), (37, 5, 3)], ids=_ids)
def test_sqdiff_mean_and_grad(dev, hb, chw, B):
    """ssm_sqdiff_mean / ssm_sqdiff_grad on the two halves of one padded buffer (the second operand is the batch-offset view phi.view(b0=B),
    as the perceptual loss passes them): float64 mean and coef[b] * (a - b); NaN scratch, sentinel around `out`, two calls bit-identical."""
    lib, st = hb.load(), hb.stream_ptr
    C, H, W = chw
    g = torch.Generator().manual_seed(C * 100 + H + W + B)
    x = torch.randn(2 * B, C, H, W, generator=g)
    coef = torch.tensor([0.3, -1.7, 2.5])[:B].clone()
    phi = hb.Planes(2 * B, C, H, W, dev).load(x.to(dev))
    a64, b64 = x[:B].double(), x[B:].double()
    want = ((a64 - b64) ** 2).flatten(1).mean(1)
    e_ref = R.rel_err(((x[:B] - x[B:]) ** 2).flatten(1).mean(1), want)
    outs = []
    for _ in range(2):
        scratch = torch.full((64 * B,), NAN, device=dev)
        buf = torch.full((B + 8,), -7.5, device=dev)
        out = buf[4:4 + B]
        hb.check(lib.ssm_sqdiff_mean(phi.view(), phi.view(b0=B), dptr(scratch), dptr(out), B, C, H, W, st()))
        b = buf.cpu()
        assert bool((b[:4] == -7.5).all()) and bool((b[4 + B:] == -7.5).all())
        outs.append(b[4:4 + B])
    assert bool(torch.isfinite(outs[0]).all()) and torch.equal(bits(outs[0]), bits(outs[1]))
    err = R.rel_err(outs[0], want)
    report("sqdiff-mean", "%s B=%d" % (chw, B), err, e_ref)
    assert err <= R.bar(e_ref), (err, e_ref)
    gout = Box(hb, dev, "planes", shape=(B, C, H, W))
    cd = coef.to(dev)
    hb.check(lib.ssm_sqdiff_grad(phi.view(), phi.view(b0=B), dptr(cd), gout.view(), B, C, H, W, st()))
    wantg = coef.double().view(B, 1, 1, 1) * (a64 - b64)
    e_ref = R.rel_err(coef.view(B, 1, 1, 1) * (x[:B] - x[B:]), wantg)
    err = R.rel_err(gout.get(), wantg)
    report("sqdiff-grad", "%s B=%d" % (chw, B), err, e_ref)
    assert err <= R.bar(e_ref) and gout.frame_is_zero(), (err, e_ref)


# ======================================================================================================================
# LeakyReLU' + the adjoint of the fused 2x2 mean
# ======================================================================================================================
def _lrelu_formula(dy, dpool, y, slope, has_act):
    """(dy + 0.25 * dpool[y/2][x/2]) * (y > 0 ? 1 : slope) in single fp32 operations, like the kernel's."""
    H, W = y.shape[2:]
    g = dy.clone() if dy is not None else torch.zeros_like(y)
    if dpool is not None:
        up = dpool.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)[:, :, :H, :W]
        g = g + 0.25 * up
    if has_act:
        g = g * torch.where(y > 0, torch.ones_like(y), torch.full_like(y, slope))
    return g


def _lrelu_inputs(B, C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    dy, y = torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g)
    dpool = torch.randn(B, C, (H + 1) // 2, (W + 1) // 2, generator=g)
    flat = y.view(-1)          # the branch's edge: +0, -0 and the smallest positive subnormal, spread over lanes and rows
    n = flat.numel()
    for i, v in enumerate((0.0, -0.0, 2.0 ** -149)):
        flat[(torch.arange(0, n, 7) + i * 2) % n] = v
    assert bool((y == 0).any()) and bool((y == 2.0 ** -149).any())
    return dy, dpool, y


# (path, W, which view is moved one column off its 16-byte boundary)
LRELU_PATHS = [("vector", 4, None), ("vector", 24, None), ("scalar", 1, None), ("scalar", 7, None), ("scalar", 26, None),
               ("scalar", 24, "dy"), ("scalar", 24, "y"), ("scalar", 24, "dz"), ("scalar", 24, "dpool")]


@pytest.mark.parametrize("path,W,off", LRELU_PATHS, ids=_ids)
def test_lrelu_bwd_paths_bit_exact(dev, hb, path, W, off):
    """ssm_lrelu_bwd picks its 4-wide kernel when W % 4 == 0 and all four views are aligned, the scalar one otherwise: each decision is
    forced (widths, one view at a time moved a column into a wider plane), with dy only / dpool only / both, has_act 0 / 1, slope 0.1 / 0
    (ReLU), C 1 / 5, and +0, -0 and the smallest subnormal planted in y.  Each output is the same three single fp32 operations as the
    torch formula (the file is built without contraction), so the bits must agree."""
    lib, st = hb.load(), hb.stream_ptr
    B, H = 2, 6
    for C in (1, 5):
        dy, dpool, y = _lrelu_inputs(B, C, H, W, seed=W * 10 + C)

        def planes(x, name):
            x0 = 1 if off == name else 0
            b, c, h, w = x.shape
            p = hb.Planes(b, c, h, w + 4 * x0, dev)
            p.full[:, :, hb.SSM_PADY:hb.SSM_PADY + h, hb.SSM_PADX + x0:hb.SSM_PADX + x0 + w] = x.to(dev)
            v = p.view(x0=x0)
            assert v.ptr % 16 == 4 * x0          # a Planes view is 16-byte aligned; one column further it is not even 8-byte aligned
            return p, v, x0
        (pdy, vdy, _), (pdp, vdp, _), (py, vy, _) = planes(dy, "dy"), planes(dpool, "dpool"), planes(y, "y")
        for src in ("dy", "dpool", "both"):
            for has_act in (0, 1):
                for slope in (0.1, 0.0):
                    pdz, vdz, x0 = planes(torch.full((B, C, H, W), NAN), "dz")
                    hb.check(lib.ssm_lrelu_bwd(vdy if src != "dpool" else hb.NULL_VIEW, vdp if src != "dy" else hb.NULL_VIEW, vy, vdz,
                                               B, C, H, W, slope, has_act, st()))
                    want = torch.zeros_like(pdz.full)
                    want[:, :, hb.SSM_PADY:hb.SSM_PADY + H, hb.SSM_PADX + x0:hb.SSM_PADX + x0 + W] = _lrelu_formula(
                        dy if src != "dpool" else None, dpool if src != "dy" else None, y, slope, has_act).to(dev)
                    assert torch.equal(bits(pdz.full), bits(want)), (C, src, has_act, slope)


@pytest.mark.parametrize("C", [8, 12, 16])
def test_lrelu_bwd_q8_twin(dev, hb, C):
    """ssm_lrelu_bwd_q8: its fp32 dz is ssm_lrelu_bwd's bit for bit; its Q8 records, decoded by ssm_hq8_to_f32, carry the value to the
    format's precision (include/ssm_hip.h: fp16(x) plus an e4m3 of (x - fp16(x)) * 2^11 - the remainder, below 2^-11 |x|, kept to half
    an e4m3 ulp = 2^-4 relative, or half its subnormal step 2^-9 once scaled back by 2^-11): |decoded - x| <= 2^-15 |x| + 2^-21."""
    lib, st = hb.load(), hb.stream_ptr
    B, H, W = 2, 6, 26
    dy, dpool, y = _lrelu_inputs(B, C, H, W, seed=C)
    pdy, pdp, py = (hb.Planes(*x.shape, dev).load(x.to(dev)) for x in (dy, dpool, y))
    for src, has_act, slope in (("both", 1, 0.1), ("dy", 1, 0.0), ("dpool", 0, 0.1)):
        vdy, vdp = (pdy.view() if src != "dpool" else hb.NULL_VIEW), (pdp.view() if src != "dy" else hb.NULL_VIEW)
        ref, dz = hb.Planes(B, C, H, W, dev), hb.Planes(B, C, H, W, dev)
        q = hb.HPlanes(B, C, H, W, dev, q8=True)
        hb.check(lib.ssm_lrelu_bwd(vdy, vdp, py.view(), ref.view(), B, C, H, W, slope, has_act, st()))
        hb.check(lib.ssm_lrelu_bwd_q8(vdy, vdp, py.view(), dz.view(), q.view(), B, C, H, W, slope, has_act, st()))
        assert float(ref.full.abs().max()) > 0 and torch.equal(bits(dz.full), bits(ref.full)), (src, has_act, slope)
        x, dec = ref.to_nchw().double().cpu(), q.to_nchw().double().cpu()
        share = float(((dec - x).abs() / (2.0 ** -15 * x.abs() + 2.0 ** -21)).max())
        print("[elementwise] lrelu-q8 C=%d %s: largest |decoded - x| / (2^-15 |x| + 2^-21) = %.3f" % (C, src, share))
        assert share <= 1.0, share


# ======================================================================================================================
# bias reduction
# ======================================================================================================================
@pytest.mark.parametrize("B,H", [(3, 1), (2, 65)], ids=_ids)
@pytest.mark.parametrize("W", [1, 11, 70])
@pytest.mark.parametrize("C", [1, 37])
def test_bias_grad_and_acc(dev, hb, C, W, B, H):
    """ssm_bias_grad overwrites a poisoned buffer, ssm_bias_grad_acc adds onto a non-zero one; padded views; B * H = 3 (one row chunk) and
    130 (three).  Error per channel relative to that channel's sum |dz|, against the float64 sum."""
    lib, st = hb.load(), hb.stream_ptr
    g = torch.Generator().manual_seed(C + W + H)
    dz = torch.randn(B, C, H, W, generator=g)
    p = hb.Planes(B, C, H, W, dev).load(dz.to(dev))
    want, scale = dz.double().sum((0, 2, 3)), dz.double().abs().sum((0, 2, 3))
    e_ref = float(((dz.sum((0, 2, 3)).double() - want).abs() / scale).max())
    db = torch.full((C + 2,), NAN, device=dev)
    hb.check(lib.ssm_bias_grad(p.view(), dptr(db[1:]), B, C, H, W, st()))
    got = db.cpu()
    assert bool(torch.isnan(got[0])) and bool(torch.isnan(got[-1])), "wrote outside db[C]"
    err = float(((got[1:-1].double() - want).abs() / scale).max())
    init = torch.randn(C, generator=g)
    acc = init.to(dev)
    hb.check(lib.ssm_bias_grad_acc(p.view(), dptr(acc), B, C, H, W, st()))
    err_acc = float(((acc.cpu().double() - (init.double() + want)).abs() / scale).max())
    report("bias-grad", "C=%d W=%d B*H=%d" % (C, W, B * H), max(err, err_acc), e_ref)
    assert err <= R.bar(e_ref), (err, e_ref)
    assert err_acc <= R.bar(e_ref), (err_acc, e_ref)


# ======================================================================================================================
# adjoint of cat + bilinear x2
# ======================================================================================================================
def _ups_ref(a, b, r, dtype):
    from oracle import ssm_oracle as O
    a = a.detach().to(dtype).requires_grad_()
    b = b.detach().to(dtype).requires_grad_() if b is not None else None
    (O.upsample2x_bilinear(a if b is None else torch.cat([a, b], 1)) * r.to(dtype)).sum().backward()
    return (a.grad,) if b is None else (a.grad, b.grad)


@pytest.mark.parametrize("h,w", [(1, 1), (5, 3), (6, 10), (23, 40)], ids=_ids)
@pytest.mark.parametrize("Ca,Cb", [(3, 2), (4, 0), (5, 6)], ids=_ids)
def test_upsample_cat_adjoint_paths(dev, hb, Ca, Cb, h, w):
    """ssm_upsample2x_cat_bwd / _mask: the two-pixel kernel (even w, aligned views) and the one-pixel kernel (odd w, or an even w with the
    hi-res gradient moved a column off its 16-byte boundary), acc_a and acc_b each off and on, against float64 autograd of
    O.upsample2x_bilinear.  The one-pixel kernel states the same association as the two-pixel one: on even widths their bits must agree.
    The mask form stays the bits of the plain form followed by ssm_lrelu_bwd, on both kernels."""
    lib, st = hb.load(), hb.stream_ptr
    B = 2
    g = torch.Generator().manual_seed(Ca * 7 + Cb + h + w)
    r = torch.randn(B, Ca + Cb, 2 * h, 2 * w, generator=g)
    ia, ib = torch.randn(B, Ca, h, w, generator=g), (torch.randn(B, Cb, h, w, generator=g) if Cb else None)
    ya = torch.randn(B, Ca, h, w, generator=g)
    ya.view(-1)[::5] = 0.0
    zeros = (torch.zeros(B, Ca, h, w), torch.zeros(B, Cb, h, w) if Cb else None)
    want = _ups_ref(*zeros, r, torch.float64)
    e_ref = max(R.rel_err(x, y) for x, y in zip(_ups_ref(*zeros, r, torch.float32), want))
    du_al = hb.Planes(B, Ca + Cb, 2 * h, 2 * w, dev).load(r.to(dev))
    du_off = hb.Planes(B, Ca + Cb, 2 * h, 2 * w + 4, dev)
    du_off.full[:, :, hb.SSM_PADY:hb.SSM_PADY + 2 * h, hb.SSM_PADX + 1:hb.SSM_PADX + 1 + 2 * w] = r.to(dev)
    pya = hb.Planes(B, Ca, h, w, dev).load(ya.to(dev))
    worst = 0.0
    for acc_a in (0, 1):
        for acc_b in ((0, 1) if Cb else (0,)):
            res = {}
            for path, vdu in (("aligned", du_al.view()), ("offset", du_off.view(x0=1))):
                da = hb.Planes(B, Ca, h, w, dev).load(ia.to(dev))
                db = hb.Planes(B, Cb, h, w, dev).load(ib.to(dev)) if Cb else None
                hb.check(lib.ssm_upsample2x_cat_bwd(vdu, da.view(), Ca, db.view() if Cb else hb.NULL_VIEW, Cb, B, h, w, acc_a, acc_b, st()))
                res[path] = (da.full.clone(), db.full.clone() if Cb else None)
                exp_a = want[0] + (ia.double() if acc_a else 0)
                err = R.rel_err(da.interior, exp_a)
                if Cb:
                    err = max(err, R.rel_err(db.interior, want[1] + (ib.double() if acc_b else 0)))
                worst = max(worst, err)
                assert err <= R.bar(e_ref), (path, acc_a, acc_b, err, e_ref)
                # frames untouched
                for pl, hh, ww in ((da, h, w),) + (((db, h, w),) if Cb else ()):
                    f = pl.full.clone()
                    f[:, :, hb.SSM_PADY:hb.SSM_PADY + hh, hb.SSM_PADX:hb.SSM_PADX + ww] = 0
                    assert not bool(f.any())
                # the mask form = plain followed by lrelu_bwd, bit for bit
                ref = hb.Planes(B, Ca, h, w, dev)
                hb.check(lib.ssm_lrelu_bwd(da.view(), hb.NULL_VIEW, pya.view(), ref.view(), B, Ca, h, w, 0.1, 1, st()))
                fa = hb.Planes(B, Ca, h, w, dev).load(ia.to(dev))
                fb = hb.Planes(B, Cb, h, w, dev).load(ib.to(dev)) if Cb else None
                hb.check(lib.ssm_upsample2x_cat_bwd_mask(vdu, fa.view(), Ca, fb.view() if Cb else hb.NULL_VIEW, Cb, pya.view(), 0.1, B, h, w,
                                                         acc_a, acc_b, st()))
                assert torch.equal(bits(fa.full), bits(ref.full)), (path, acc_a, acc_b)
                if Cb:
                    assert torch.equal(bits(fb.full), bits(db.full)), (path, acc_a, acc_b)
            assert torch.equal(bits(res["aligned"][0]), bits(res["offset"][0])), "the two kernels disagree on da"
            if Cb:
                assert torch.equal(bits(res["aligned"][1]), bits(res["offset"][1])), "the two kernels disagree on db"
    report("upsample-adj", "Ca=%d Cb=%d %dx%d" % (Ca, Cb, h, w), worst, e_ref)


# ======================================================================================================================
# MaxPool2d(2, 2)
# ======================================================================================================================
@pytest.mark.parametrize("Wh", [1, 65])
@pytest.mark.parametrize("C", [1, 6])
def test_maxpool_ties_bit_exact(dev, hb, C, Wh):
    """Inputs quantised to {-0, +0, 1, 2}: ties in every window position, all-equal windows, +0 against -0.  Forward and backward must be
    torch.nn.functional.max_pool2d's bits (the first maximum of the row-major scan wins, value and gradient).
    Regression case: the forward took fmaxf, which orders -0 below +0, and returned +0 for a window whose first zero is -0."""
    lib, st = hb.load(), hb.stream_ptr
    B, Hh = 2, 5
    H, W = 2 * Hh, 2 * Wh
    g = torch.Generator().manual_seed(C * 10 + Wh)
    x = torch.randint(0, 3, (B, C, H, W), generator=g).float()
    x = torch.where((x == 0) & (torch.rand(x.shape, generator=g) < 0.5), torch.full_like(x, -0.0), x)
    x[:, :, 0:2, 0:2] = 1.0                      # all-equal windows
    x[:, :, 2:4, 0:2] = 0.0
    x[:, :, 4:6, 0:2] = -0.0
    x[:, :, 6:8, 0:2] = torch.tensor([[-0.0, 0.0], [0.0, -0.0]])
    x[:, :, 8:10, 0:2] = torch.tensor([[0.0, -0.0], [-0.0, 0.0]])
    dy = torch.randn(B, C, Hh, Wh, generator=g)
    xr = x.clone().requires_grad_()
    want = torch.nn.functional.max_pool2d(xr, kernel_size=2, stride=2)
    (want * dy).sum().backward()
    px, pdy = hb.Planes(B, C, H, W, dev).load(x.to(dev)), hb.Planes(B, C, Hh, Wh, dev).load(dy.to(dev))
    py, pdx = Box(hb, dev, "planes", shape=(B, C, Hh, Wh)), Box(hb, dev, "planes", shape=(B, C, H, W))
    hb.check(lib.ssm_maxpool2_fwd(px.view(), py.view(), B, C, H, W, st()))
    hb.check(lib.ssm_maxpool2_bwd(px.view(), pdy.view(), pdx.view(), B, C, H, W, st()))
    assert torch.equal(bits(py.get()), bits(want.detach())), "forward"
    assert torch.equal(bits(pdx.get()), bits(xr.grad)), "backward"
    assert py.frame_is_zero() and pdx.frame_is_zero()


# ======================================================================================================================
# recurrent cells, forward and adjoint
# ======================================================================================================================
def _pre(shape, g, saturate):
    x = torch.randn(shape, generator=g) * 2
    if saturate:          # a tenth of the pre-activations at +-30: sigmoid and tanh at their fp32 limits
        m = torch.rand(shape, generator=g) < 0.1
        x = torch.where(m, torch.where(torch.rand(shape, generator=g) < 0.5, torch.full_like(x, 30.0), torch.full_like(x, -30.0)), x)
    return x


def _cmp(group, case, names, got, fn, worst):
    """got: list of cpu tensors; fn(dtype) -> tuple of references.  Entries whose float64 value is not above 1e-30 in magnitude are left
    out (a saturated gate's derivative underflows in fp32 by design)."""
    want, lo = fn(torch.float64), fn(torch.float32)
    for name, gt, w, l in zip(names, got, want, lo):
        assert bool(torch.isfinite(gt).all()), name
        keep = w.abs() > 1e-30
        err, e_ref = R.rel_err(gt, w, keep), R.rel_err(l, w, keep)
        worst[:] = max(worst, [err / R.bar(e_ref), err, e_ref])
        assert err <= R.bar(e_ref), (group, case, name, err, e_ref)


@pytest.mark.parametrize("saturate", [False, True], ids=["randn2", "saturated"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("H,W", [(1, 1), (5, 7), (11, 11)], ids=_ids)
@pytest.mark.parametrize("Hc", [8, 24])
def test_convlstm_cell_and_adjoint(dev, hb, Hc, H, W, layout, saturate):
    lib, st = hb.load(), hb.stream_ptr
    B = 3
    g = torch.Generator().manual_seed(Hc + H + W)
    gx, gh = _pre((B, 4 * Hc, H, W), g, saturate), _pre((B, 4 * Hc, H, W), g, False) * 0.5
    cp, dh, dcn = (torch.randn(B, Hc, H, W, generator=g) for _ in range(3))
    mk = lambda x: Box(hb, dev, layout, x)     # noqa: E731
    bgx, bgh, bcp, bdh, bdcn = mk(gx), mk(gh), mk(cp), mk(dh), mk(dcn)
    worst = [0.0, 0.0, 0.0]
    case = "Hc=%d %dx%d %s %s" % (Hc, H, W, layout, "sat" if saturate else "")
    for first in (False, True):          # first step: gates_h and c_prev are NULL views (h_0 = c_0 = 0)
        pre = gx if first else gx + gh          # one fp32 addition, as in the kernel
        c0 = None if first else cp
        cn, hf = Box(hb, dev, layout, shape=(B, Hc, H, W)), Box(hb, dev, layout, shape=(B, Hc, H, W))
        hb.check(lib.ssm_convlstm_cell_fwd(bgx.view(), hb.NULL_VIEW if first else bgh.view(), hb.NULL_VIEW if first else bcp.view(), cn.view(),
                                           hf.view(), hb.NULL_HVIEW, B, Hc, H, W, 0, st()))
        _cmp("lstm", case, ("h", "c_next"), [hf.get(), cn.get()],
             lambda dt: R.lstm_cell(pre.to(dt), None if c0 is None else c0.to(dt)), worst)
        assert hf.frame_is_zero() and cn.frame_is_zero()
        for with_dc in (True, False):          # dc_next NULL = 0 (the last step of the sequence)
            dg, dcp = Box(hb, dev, layout, shape=(B, 4 * Hc, H, W)), Box(hb, dev, layout, shape=(B, Hc, H, W))
            hb.check(lib.ssm_convlstm_cell_bwd(bgx.view(), hb.NULL_VIEW if first else bgh.view(), hb.NULL_VIEW if first else bcp.view(),
                                               bdh.view(), bdcn.view() if with_dc else hb.NULL_VIEW, dg.view(), dcp.view(), B, Hc, H, W, st()))
            czero = torch.zeros_like(cp) if first else cp          # the zero state still has a gradient: d c_prev = d c' * sigmoid(f)
            _cmp("lstm", case, ("dgates", "dc_prev"), [dg.get(), dcp.get()],
                 lambda dt: R.grads(R.lstm_cell, (pre, czero), (dh, dcn if with_dc else None), dt)[1], worst)
            assert dg.frame_is_zero() and dcp.frame_is_zero()
    report("lstm-cell", case, worst[1], worst[2])


@pytest.mark.parametrize("saturate", [False, True], ids=["randn2", "saturated"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("H,W", [(1, 1), (5, 7), (11, 11)], ids=_ids)
@pytest.mark.parametrize("Hc", [8, 24])
def test_convgru_cells_and_adjoints(dev, hb, Hc, H, W, layout, saturate):
    lib, st = hb.load(), hb.stream_ptr
    B, SENT = 3, -123.25
    g = torch.Generator().manual_seed(Hc * 3 + H + W)
    gx, gh = _pre((B, 2 * Hc, H, W), g, saturate), _pre((B, 2 * Hc, H, W), g, False) * 0.5
    cx, ch = _pre((B, Hc, H, W), g, saturate), _pre((B, Hc, H, W), g, False) * 0.5
    hp, drh, dhn = (torch.randn(B, Hc, H, W, generator=g) for _ in range(3))
    mk = lambda x: Box(hb, dev, layout, x)     # noqa: E731
    bgx, bgh, bcx, bch, bhp, bdrh, bdhn = mk(gx), mk(gh), mk(cx), mk(ch), mk(hp), mk(drh), mk(dhn)
    gates, cand = gx + gh, cx + ch          # the summed pre-activations the adjoints take
    bg, bc = mk(gates), mk(cand)
    worst = [0.0, 0.0, 0.0]
    case = "Hc=%d %dx%d %s %s" % (Hc, H, W, layout, "sat" if saturate else "")
    new = lambda n: Box(hb, dev, layout, shape=(B, n, H, W))     # noqa: E731
    # reset half, forward and adjoint
    rh = new(Hc)
    hb.check(lib.ssm_convgru_reset_fwd(bgx.view(), bgh.view(), bhp.view(), rh.view(), hb.NULL_HVIEW, B, Hc, H, W, 0, st()))
    _cmp("gru", case, ("rh",), [rh.get()], lambda dt: (R.gru_reset(gates.to(dt), hp.to(dt)),), worst)
    dgt, dhp = Box(hb, dev, layout, shape=(B, 2 * Hc, H, W), fill=SENT), new(Hc)
    hb.check(lib.ssm_convgru_reset_bwd(bg.view(), bhp.view(), bdrh.view(), dgt.view(), dhp.view(), B, Hc, H, W, st()))
    got = dgt.get()
    assert bool((got[:, Hc:] == SENT).all()), "reset_bwd owns dgates[0:Hc] only"

    def reset_ref(dt):
        _, (dg_, dh_) = R.grads(R.gru_reset, (gates, hp), (drh,), dt)
        return dg_[:, :Hc], dh_
    _cmp("gru", case, ("dgamma", "dh_prev"), [got[:, :Hc], dhp.get()], reset_ref, worst)
    # update half, forward and adjoint, with a state and at the first step (gates_h, cand_h, h_prev / dh_prev NULL)
    for first in (False, True):
        gts, cnd, h0 = (gx, cx, None) if first else (gates, cand, hp)
        hn = new(Hc)
        N = hb.NULL_VIEW
        hb.check(lib.ssm_convgru_update_fwd(bgx.view(), N if first else bgh.view(), bcx.view(), N if first else bch.view(),
                                            N if first else bhp.view(), hn.view(), hb.NULL_HVIEW, B, Hc, H, W, 0, st()))
        _cmp("gru", case, ("h",), [hn.get()], lambda dt: (R.gru_update(gts.to(dt), cnd.to(dt), None if h0 is None else h0.to(dt)),), worst)
        dgt, dcd, dhp = Box(hb, dev, layout, shape=(B, 2 * Hc, H, W), fill=SENT), new(Hc), new(Hc)
        hb.check(lib.ssm_convgru_update_bwd((bgx if first else bg).view(), (bcx if first else bc).view(), N if first else bhp.view(), bdhn.view(),
                                            dgt.view(), dcd.view(), N if first else dhp.view(), B, Hc, H, W, st()))
        got = dgt.get()
        assert bool((got[:, :Hc] == SENT).all()), "update_bwd owns dgates[Hc:2Hc] only"
        if first:
            assert bool(torch.isnan(dhp.get()).all())          # NULL view: nothing written

        def update_ref(dt):
            _, gr = R.grads(R.gru_update, (gts, cnd, h0), (dhn,), dt)
            return (gr[0][:, Hc:], gr[1]) + (() if first else (gr[2],))
        _cmp("gru", case, ("dbeta", "dcand", "dh_prev"), [got[:, Hc:], dcd.get()] + ([] if first else [dhp.get()]), update_ref, worst)
        assert dgt.frame_is_zero() and dcd.frame_is_zero() and hn.frame_is_zero()
    report("gru-cell", case, worst[1], worst[2])
