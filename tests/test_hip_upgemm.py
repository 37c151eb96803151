"""GPU parity of the decoder step conv3x3(upsample2x(cat[a, b])) (scripts/models/flow_computation.py:244-247) evaluated as a 1x1 GEMM at low
resolution followed by the nine taps after the upsample (csrc/ssm_upgemm.hip), against the CPU oracle's upsample + direct convolution.
Bar 5e-5 like every other form (outputs of magnitude ~1; the form's own rounding is ~2e-6, tests/test_upgemm_cpu.py): a miss is a bug.
Both tile configurations of the GEMM are forced through ssm_upgemm_force_kind; every ragged shape overshoots a tile on both axes.  (The GEMM
stays under 64 KiB of LDS, so there is no per-device opt-in to race on: no two-thread case.)"""
import pytest
import torch

pytestmark = pytest.mark.gpu
BAR = 5e-5
KINDS = ["G16", "G8"]          # low-res pixels per workgroup: 16 x 16, 8 x 16


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _unforce():
    yield
    from ssm_amd import hipbind as hb
    hb.load().ssm_upgemm_force_kind(-1)


def _force(kind):
    from ssm_amd import hipbind as hb
    n = hb.load().ssm_upgemm_force_kind(KINDS.index(kind))
    assert n == len(KINDS), "tile-configuration list of the test is out of date (%d in the library)" % n


def _problem(g, B, h, w, c1, c2, cout, broadcast=False):
    a = torch.randn(B, c1, h, w, generator=g)
    b = torch.randn(1 if broadcast else B, c2, h, w, generator=g) if c2 else None
    wt = torch.randn(cout, c1 + c2, 3, 3, generator=g) / ((c1 + c2) * 9) ** 0.5
    bias = torch.randn(cout, generator=g) * 0.1
    return a, b, wt, bias


def _cat(a, b):
    return a if b is None else torch.cat([a, b.expand(a.shape[0], -1, -1, -1)], 1)


def _want(O, a, b, wt, bias):
    """The reference of every case: the oracle's upsample of the concat, then its direct 3x3 convolution + LeakyReLU."""
    return O.conv2d_lrelu(O.upsample2x_bilinear(_cat(a, b)), wt, bias)


def _run(hb, dev, a, b, wt, bias, lrelu=True, add=None, add_div=1, poison=None):
    """-> (output NCHW on the CPU, the output Planes).  poison: value written behind the sources' last planes and over the whole scratch set
    before the launch."""
    B, c1, h, w = a.shape
    c2 = 0 if b is None else b.shape[1]
    H, W, cout = 2 * h, 2 * w, wt.shape[0]
    pa = hb.Planes(B, c1, h, w, dev).load(a.to(dev))
    pb = hb.Planes(b.shape[0], c2, h, w, dev).load(b.to(dev)) if c2 else None
    pk = hb.PackedUpGemm(wt.to(dev), bias.to(dev), B, H, W)
    y = hb.Planes(B, cout, H, W, dev)
    if poison is not None:
        pa.buf[pa.full.numel():] = poison
        if pb is not None:
            pb.buf[pb.full.numel():] = poison
        pk.scratch = torch.full((pk.scratch_floats(B, H, W),), poison, dtype=torch.float32, device=dev)
    padd = hb.Planes(add.shape[0], cout, H, W, dev).load(add.to(dev)) if add is not None else None
    hb.conv2d_ups_upgemm(pa.view(), c1, pb.view(broadcast=b.shape[0] == 1 and B > 1) if c2 else None, c2, pk, y.view(), B, H, W, lrelu=lrelu,
                         add=padd.view() if padd is not None else None, add_div=add_div)
    return y.to_nchw().cpu(), y


def _ring_and_interior(e):
    """max of an error map on the border ring (rows / columns 0, 1, -2, -1: where edge clamp and zero padding differ) and off it."""
    m = torch.zeros(e.shape[-2:], dtype=torch.bool)
    m[:2], m[-2:], m[:, :2], m[:, -2:] = True, True, True, True
    ring = float(e[..., m].max())
    inner = float(e[..., ~m].max()) if bool((~m).any()) else 0.0
    return ring, inner


@pytest.mark.parametrize("channels", [(16, 16), (16, 8)], ids=["whole-chunks", "ragged-chunks"])
@pytest.mark.parametrize("kind", KINDS)
def test_every_configuration_small_odd_and_ragged_maps(dev, kind, channels):
    from oracle import ssm_oracle as O
    from ssm_amd import hipbind as hb
    g = torch.Generator().manual_seed(10 * KINDS.index(kind) + channels[1])
    _force(kind)
    c1, c2 = channels
    for h, w in ((3, 5), (7, 9), (23, 40)):
        a, b, wt, bias = _problem(g, 2, h, w, c1, c2, 64, broadcast=True)
        want = _want(O, a, b, wt, bias)
        got, y = _run(hb, dev, a, b, wt, bias)
        ring, inner = _ring_and_interior((got - want).abs())
        print("upgemm %s %dx%d c=%d+%d: ring %.3e interior %.3e" % (kind, h, w, c1, c2, ring, inner))
        assert ring < BAR, "%s %dx%d: border ring %.3e" % (kind, h, w, ring)
        assert inner < BAR, "%s %dx%d: interior %.3e" % (kind, h, w, inner)
        full = y.full.cpu().clone()
        full[:, :, hb.SSM_PADY:hb.SSM_PADY + 2 * h, hb.SSM_PADX:hb.SSM_PADX + 2 * w] = 0
        assert float(full.abs().max()) == 0.0, "%s wrote outside the interior" % kind


@pytest.mark.parametrize("c1,c2,cout,h,w,broadcast", [(8, 4, 32, 7, 9, False), (20, 0, 64, 7, 9, False), (512, 512, 64, 6, 10, True)],
                         ids=["cin12=8+4", "cin20", "cin1024-broadcast"])
def test_channel_counts(dev, c1, c2, cout, h, w, broadcast):
    from oracle import ssm_oracle as O
    from ssm_amd import hipbind as hb
    g = torch.Generator().manual_seed(c1 + c2)
    a, b, wt, bias = _problem(g, 2, h, w, c1, c2, cout, broadcast=broadcast)
    want = _want(O, a, b, wt, bias)
    got, _ = _run(hb, dev, a, b, wt, bias)
    e = float((got - want).abs().max())
    print("upgemm cin %d+%d cout %d: %.3e" % (c1, c2, cout, e))
    assert e < BAR, e


def test_unsupported_cout_is_refused_and_the_plan_falls_back(dev):
    from ssm_amd import engine as E
    from ssm_amd import hipbind as hb
    assert hb.upgemm_supported(64, 32, 16, 16) and hb.upgemm_supported(64, 64, 16, 16)
    assert not hb.upgemm_supported(64, 48, 16, 16) and not hb.upgemm_supported(64, 32, 16, 16, k=5)
    with pytest.raises(RuntimeError, match="unsupported"):
        hb.PackedUpGemm(torch.zeros(48, 64, 3, 3, device=dev), torch.zeros(48, device=dev), 1, 16, 16)
    v = hb.Planes(1, 64, 8, 8, dev).view()
    rc = hb.load().ssm_upgemm_conv2d_ups_add_fwd(v, 64, hb.NULL_VIEW, 0, v.ptr, v.ptr, v, v, hb.NULL_VIEW, 1, 1, 16, 16, 48, 0.1, 0, None)
    assert rc == -1 and b"unsupported" in hb.load().ssm_last_error_string()
    old = E.UPGEMM
    E.UPGEMM = "conv8a"
    try:
        assert E.choose_algo("conv8a", 64, 32, 3, 1, 16, 16, True, True, True) == "upgemm"
        assert E.choose_algo("conv8a", 64, 48, 3, 1, 16, 16, True, True, True) != "upgemm"
    finally:
        E.UPGEMM = old


@pytest.mark.parametrize("lrelu", [True, False])
@pytest.mark.parametrize("add_div", [1, 7])
def test_pre_activation_addend(dev, add_div, lrelu):
    from oracle import ssm_oracle as O
    from ssm_amd import hipbind as hb
    g = torch.Generator().manual_seed(30 + add_div)
    B, h, w = 7, 5, 12
    a, b, wt, bias = _problem(g, B, h, w, 16, 0, 32)
    add = torch.randn(B // add_div, 32, 2 * h, 2 * w, generator=g)
    pre = O.conv2d(O.upsample2x_bilinear(_cat(a, b)), wt, bias) + add.repeat_interleave(add_div, 0)
    want = torch.where(pre >= 0, pre, pre * O.LRELU_SLOPE) if lrelu else pre
    got, _ = _run(hb, dev, a, b, wt, bias, lrelu=lrelu, add=add, add_div=add_div)
    e = float((got - want).abs().max())
    assert e < BAR, "add_div %d lrelu %s: %.3e" % (add_div, lrelu, e)


def test_scale_invariance(dev):
    """Inputs x 64, filters x 1/64: linear fp32 arithmetic - the same relative error (bar scaled with the output, as
    test_wino4_deep_channels_and_scale_invariance does)."""
    from oracle import ssm_oracle as O
    from ssm_amd import hipbind as hb
    g = torch.Generator().manual_seed(5)
    a, b, wt, bias = _problem(g, 2, 12, 20, 128, 128, 64)
    for sx, sw in ((1.0, 1.0), (64.0, 1.0 / 64)):
        want = _want(O, a * sx, b * sx, wt * sw, bias)
        got, _ = _run(hb, dev, a * sx, b * sx, wt * sw, bias)
        e = float((got - want).abs().max())
        assert e < BAR * sx * sw, "scale %g x %g: %.3e" % (sx, sw, e)


@pytest.mark.parametrize("poison", [float("nan"), 3.0e30])
@pytest.mark.parametrize("kind", KINDS)
def test_overshoot_reads_nothing_it_should_not(dev, kind, poison):
    """The memory behind the sources' last planes and the WHOLE scratch set are poisoned before the launch: the GEMM's tile overshoot
    must never reach a stored value, and the combine pass must read no scratch element the GEMM did not write."""
    from oracle import ssm_oracle as O
    from ssm_amd import hipbind as hb
    g = torch.Generator().manual_seed(77)
    _force(kind)
    for (h, w), (c1, c2) in (((7, 9), (16, 16)), ((23, 40), (8, 4)), ((16, 16), (16, 0))):
        a, b, wt, bias = _problem(g, 1, h, w, c1, c2, 32)
        want = _want(O, a, b, wt, bias)
        got, y = _run(hb, dev, a, b, wt, bias, poison=poison)
        assert bool(torch.isfinite(got).all()), "%s %dx%d: non-finite outputs (poison %g reached an output)" % (kind, h, w, poison)
        e = float((got - want).abs().max())
        assert e < BAR, "%s %dx%d: %.3e" % (kind, h, w, e)
        full = y.full.cpu().clone()
        full[:, :, hb.SSM_PADY:hb.SSM_PADY + 2 * h, hb.SSM_PADX:hb.SSM_PADX + 2 * w] = 0
        assert float(full.abs().max()) == 0.0, "%s wrote outside the interior" % kind
