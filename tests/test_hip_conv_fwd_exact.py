"""The fp32 FORWARD convolution forms whose arithmetic is exact on integer operands, held to BIT EQUALITY (torch.equal, no tolerance)
with the float64 oracle: csrc/ssm_conv.hip (all 15 tile kinds, split-K, final_conv in both forms), csrc/ssm_wino.hip (all 12 kinds,
split-K, fused upsample) and csrc/ssm_upgemm.hip (both kinds).  References and case tables: tests/conv_refs.py (budgets asserted on the
CPU by tests/test_conv_refs_cpu.py); the style of tests/test_hip_wgrad_exact.py.

Why each form is exact on integer operands inside conv_refs.exactness_budget (read from the kernels):
  ssm_conv.hip    products of integers summed by v_mfma_f32_32x32x2_f32 into fp32 accumulators, the bias as one more MFMA k-step (bias x 1),
                  the addend as the accumulators' start: integers below 2^24 in any order.  Fused upsample: the expander forms
                  xa v0 + xb v1 with (xa, xb) in {(1, 0), (.75, .25)} per axis - multiples of 1/4, then of 1/16, exact with or without FMA
                  contraction - and the border masks are 0 / 1.  Split-K (ssm_conv2d_splitk_fwd + ssm_splitk_finish_fwd) adds exact partial
                  sums.  final_conv: fmaf chains (vector-ALU form) / v_mfma_f32_4x4x1 (matrix form) of the same integers.
  ssm_wino.hip    U = G g G^T with G = [1 0 0; .5 .5 .5; .5 -.5 .5; 0 0 1] is evaluated in fp32 by the pack kernel as 0.5 * (g0 +- g1 + g2):
                  sums of small integers, halved twice - multiples of 1/4, exact.  B^T d B has entries 0, +-1 (4-term sums of the inputs or
                  of their exact 1/16-granular upsample), the 16 frequencies are MFMA sums of multiples of 1/4 (1/64 with the upsample), the
                  bias starts the accumulator of frequency (1, 1), which A^T M A (entries 0, +-1; 9-term sums) adds once to every output.
  ssm_upgemm.hip  the GEMM sums integer products per tap at low resolution; the combine pass weights them with .75 / .25 per axis
                  (products (0.75 mt) c with mt in {0, 1}) - multiples of 1/16 of sums the budget bounds - then adds bias and addend.
  Epilogues       fmaxf(t, t * slope) with slope = 0.1f (1.0f without activation): t itself for t >= 0, ONE rounding of t * 0.1f for t < 0 =
                  conv_refs.lrelu_once; the mask epilogue multiplies by (m > 0 ? 1 : 0.1f): one rounding as well.  The fused 2x2 mean is
                  ((y00 + y10) + (y01 + y11)) * 0.25 of the ACTIVATED outputs: exact when all four are multiples of the granule (the run whose
                  integer bias lifts every pre-activation to >= 0), three adds and one multiply of rounded values otherwise - held to
                  4 * 2^-24 * sum |y| there, the only bound of this module.
  No form had to be moved to tests/test_hip_conv_fwd_oneterm.py.

Cases (conv_refs.exact_case_table).  Per kind, (B, H, W) = (2,22,44) (1,23,40) (3,6,2) (1,9,131) (1,5,7) (1,1,1) (2,32,64) (3,12,20) - tiles
overshoot on both axes, maps smaller than a tile, odd sizes, one multi-tile even map, one batch of 3 for add_div = 3 - with 16 + 8 input
channels (two sources, each a channel window of a wider Planes whose other channels hold NaN) -> 40 outputs (a ragged cout block), operands
uniform on {-3..3}; the direct form's addend runs use 128 outputs (its addend is read in whole cout blocks).  Fused upsample: the same
list as LOW-res shapes, second source batch-broadcast, operands on {-2..2}.  Deep (the k-loop's double buffer): 512 -> 128 (3x3), 64 -> 64
(5x5), 32 -> 32 (7x7) at 2 x 22 x 22; 256 -> 128 at 2 x 11 x 11 low-res for the fused upsample.  Split-K: 512 -> 128 at 2 x 22 x 22
(F(2x2,3x3)), the direct form's on 2 x 11 x 11.  final_conv: 32 -> 4 / 5 / 8 / 1 on the four maps of test_final_conv_both_forms_vs_oracle.
Per case: lrelu off == z; lrelu on == lrelu_once(z); pre-activation addend with add_div 1 and 3; mask epilogue (F(2x2,3x3): the direct
form and the GEMM form have none); Planes output with the frame asserted zero, plain NCHW output into a buffer of 7.0 (F(2x2,3x3): even
widths - it stores row pairs and refuses other views; the GEMM form: output widths that are multiples of 4 - 88, 80, 4, 128, 40 of the
list - since its entry point asks for a 16-byte-aligned pointer and strides that are multiples of 4, which a contiguous NCHW buffer of
such a width has, and its combine pass stores whole 16-byte pieces or single floats below the row's end); the fused 2x2 mean in both
runs (even maps, kinds that have it).
Negative control, one per source file: ONE non-zero input pixel of the last row zeroed on the GPU side only - the result must differ.

What was found (MI355X).  Every form, every kind, every case and option above: bit-equal - nothing needed a bound beyond the stated
one of the mixed-sign fused mean, and no kernel had to be changed.  Negative controls (one non-zero pixel of the last input row zeroed on
the GPU side only, 2 x 22 x 44): ssm_conv.hip 133 outputs differ, ssm_wino.hip 133, ssm_upgemm.hip (low-res pixel) 1982 - bit equality
sees a single pixel.  The GEMM form's NCHW runs (output widths 88, 80, 4, 128, 40, both kinds) are bit-equal too.  The fused-upsample F(2x2,3x3) of 256 channels at 2 x 11 x 11 low-res runs split (KS = 4) and is bit-equal too.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_refs as R  # noqa: E402

pytestmark = pytest.mark.gpu

CONV_KINDS = ["K7", "K5", "K3N32", "K3N64", "K3N128", "K3N128S", "K3N64T", "K3N32T", "K3N128G", "K3N64G", "K3N64GS", "K3N32G",
              "K3N32GS", "K5G", "K7G"]
CONV_KS = {"K7": 7, "K7G": 7, "K5": 5, "K5G": 5}
CONV_NO_POOL_UPS = {"K3N32T"}          # odd row tile: no fused pool / upsample
WINO_KINDS = ["W64A", "W32A", "W128A", "W64G", "W128G", "W64H", "W128H", "V32A", "V32H", "V32G", "V64A", "V64G"]
UPGEMM_KINDS = ["G16", "G8"]
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _unforce():
    yield
    from ssm_amd import hipbind as hb
    lib = hb.load()
    lib.ssm_conv_force_kind(-1)
    lib.ssm_wino_force_kind(-1)
    lib.ssm_upgemm_force_kind(-1)


def _force(fn, kinds, kind):
    n = fn(kinds.index(kind))
    assert n == len(kinds), "tile-configuration list of the test is out of date (%d in the library)" % n


def _window(hb, t, dev, c0=3, extra=5):
    """t as channels [c0, c0 + C) of a wider Planes whose other channels are NaN -> (planes, view of the window)."""
    B, C, H, W = t.shape
    p = hb.Planes(B, C + extra, H, W, dev)
    p.interior[:] = NAN
    p.interior[:, c0:c0 + C] = t.to(dev)
    return p


def _frame_is_zero(hb, y, H, W):
    full = y.full.clone()
    full[:, :, hb.SSM_PADY:hb.SSM_PADY + H, hb.SSM_PADX:hb.SSM_PADX + W] = 0
    return not bool(full.any())


class Runner:
    """One exact problem on the GPU: sources loaded once, launches through `launch(av, c1, bv, c2, pk, yview, poolview, **kw)`."""

    def __init__(self, hb, dev, p, pack, launch, bcast=False):
        self.hb, self.dev, self.p, self.pack, self.launch = hb, dev, p, pack, launch
        self.B, self.c1 = p["a"].shape[:2]
        self.c2 = 0 if p["b"] is None else p["b"].shape[1]
        self.cout = p["w"].shape[0]
        self.H, self.W = p["out_hw"]
        self.pa = _window(hb, p["a"], dev)
        self.pb = _window(hb, p["b"], dev, c0=2, extra=3) if self.c2 else None
        self.bcast = bcast
        self.pk = pack(p["w"].to(dev), p["bias"].to(dev))

    def views(self):
        return self.pa.view(c0=3), (self.pb.view(c0=2, broadcast=self.bcast) if self.c2 else None)

    def run(self, pk=None, pool=False, nchw=False, **kw):
        """-> (y NCHW on the CPU, pooled or None); asserts the frame (Planes) stays zero."""
        hb = self.hb
        av, bv = self.views()
        yp = hb.Planes(self.B, self.cout, max(self.H // 2, 1), max(self.W // 2, 1), self.dev) if pool else None
        if nchw:
            y = torch.full((self.B, self.cout, self.H, self.W), 7.0, device=self.dev)
            self.launch(av, self.c1, bv, self.c2, pk or self.pk, hb.view_of(y), yp.view() if pool else None, **kw)
            out = y.cpu()
        else:
            y = hb.Planes(self.B, self.cout, self.H, self.W, self.dev)
            self.launch(av, self.c1, bv, self.c2, pk or self.pk, y.view(), yp.view() if pool else None, **kw)
            out = y.to_nchw().cpu()
            assert _frame_is_zero(hb, y, self.H, self.W), "wrote outside the interior"
        return out, (yp.to_nchw().cpu() if pool else None)


def _check_plain(r, name, pool_ok, nchw_ok=True, mask=False):
    """lrelu off / on, NCHW output, the fused mean in both runs, the mask epilogue."""
    from oracle import ssm_oracle as O
    p = r.p
    z = p["z"]
    got, _ = r.run(lrelu=False)
    assert torch.equal(got, z), "%s: lrelu off, %d outputs differ" % (name, int((got != z).sum()))
    act = R.lrelu_once(z)
    pool = pool_ok and r.H % 2 == 0 and r.W % 2 == 0
    got, gp = r.run(lrelu=True, pool=pool)
    assert torch.equal(got, act), "%s: lrelu on, %d outputs differ" % (name, int((got != act).sum()))
    if pool:          # mixed signs: three adds and one multiply of rounded values
        err, bound = (gp.double() - O.avg_pool2(act.double())).abs(), R.pool_bound(act)
        assert bool((err <= bound).all()), "%s: fused mean, mixed signs: %.3e over the bound" % (name, float((err - bound).max()))
        pk_pos = r.pack(p["w"].to(r.dev), (p["bias"] + p["lift"]).to(r.dev))
        got, gp = r.run(pk=pk_pos, lrelu=True, pool=True)
        assert torch.equal(got, p["z_pos"]), "%s: lifted run" % name
        assert torch.equal(gp, R.exact_f32(O.avg_pool2(p["z_pos"].double()))), "%s: fused mean of non-negative outputs is not exact" % name
    if nchw_ok:
        got, _ = r.run(lrelu=True, nchw=True)
        assert torch.equal(got, act), "%s: NCHW output into a buffer of 7.0" % name
    if mask:
        m = p["add"][1]
        pm = r.hb.Planes(*m.shape, r.dev).load(m.to(r.dev))
        got, _ = r.run(lrelu=False, add=pm.view(), mask=True)
        want = torch.where(m > 0, z, z * torch.tensor(0.1))
        assert torch.equal(got, want), "%s: mask epilogue" % name


def _check_add(r, name):
    p = r.p
    for div, add in p["add"].items():
        pa = r.hb.Planes(*add.shape, r.dev).load(add.to(r.dev))
        got, _ = r.run(lrelu=True, add=pa.view(), add_div=div)
        want = R.lrelu_once(p["z_add"][div])
        assert torch.equal(got, want), "%s: addend, add_div %d: %d outputs differ" % (name, div, int((got != want).sum()))
    assert p["add"], name


def _negative_control(r, name):
    """One non-zero pixel of the last input row zeroed on the GPU side only: bit equality must see it."""
    a = r.p["a"]
    nzx = torch.nonzero(a[-1, -1, -1])
    assert nzx.numel(), "the last row of the last channel is all zero"
    r.pa.interior[-1, 3 + a.shape[1] - 1, -1, int(nzx[0])] = 0.0
    got, _ = r.run(lrelu=False)
    diff = int((got != r.p["z"]).sum())
    print("[fwd_exact] negative control %s: %d outputs differ" % (name, diff))
    assert diff > 0, "%s: a zeroed input pixel went unnoticed" % name


def _problem(k, cout, shape, ups=False):
    B, H, W = shape
    if ups:
        return R.exact_problem(3, R.EXACT_C1, R.EXACT_C2, cout, B, H, W, True, True, "wino", 2)
    return R.exact_problem(k, R.EXACT_C1, R.EXACT_C2, cout, B, H, W, False, False, "wino" if k == 3 else "direct")


# ---- csrc/ssm_conv.hip ---------------------------------------------------------------------------------------------------------------
def _conv_runner(hb, dev, p, B, H, W, pool, ups=False, bcast=False):
    def pack(w, b, pool=pool):
        return hb.PackedConv(w, b, B, H, W, pool=pool, ups=ups)

    def launch(av, c1, bv, c2, pk, y, yp, **kw):
        if ups:
            return hb.conv2d_ups(av, c1, bv, c2, pk, y, B, H, W, **kw)
        return hb.conv2d(av, c1, bv, c2, pk, y, yp, B, H, W, **kw)
    return Runner(hb, dev, p, pack, launch, bcast)


@pytest.mark.parametrize("kind", CONV_KINDS)
def test_direct_every_kind_exact(dev, kind):
    from ssm_amd import hipbind as hb
    k = CONV_KS.get(kind, 3)
    _force(hb.load().ssm_conv_force_kind, CONV_KINDS, kind)
    pool_ok = kind not in CONV_NO_POOL_UPS
    for shape in R.EXACT_SHAPES:
        B, H, W = shape
        name = "%s %dx%dx%d" % (kind, B, H, W)
        pool = pool_ok and H % 2 == 0 and W % 2 == 0
        assert hb.conv_plan(k, 24, R.EXACT_COUT, B, H, W, pool)[0] == CONV_KINDS.index(kind)
        # the packed filter depends on the fused pool through the plan only: the runner is built with the setting it is launched with
        _check_plain(_conv_runner(hb, dev, _problem(k, R.EXACT_COUT, shape), B, H, W, pool), name, pool)
        _check_add(_conv_runner(hb, dev, _problem(k, R.EXACT_COUT_ADD, shape), B, H, W, False), name)
    cin, cout, B, H, W = R.DEEP_CASES[k]
    p = R.exact_problem(k, cin, 0, cout, B, H, W, False, False, "wino" if k == 3 else "direct")
    _check_plain(_conv_runner(hb, dev, p, B, H, W, False), "%s deep %d->%d" % (kind, cin, cout), False)


@pytest.mark.parametrize("kind", [k for k in CONV_KINDS if k not in CONV_KS and k not in CONV_NO_POOL_UPS])
def test_direct_every_kind_fused_upsample_exact(dev, kind):
    from ssm_amd import hipbind as hb
    _force(hb.load().ssm_conv_force_kind, CONV_KINDS, kind)
    for shape in R.EXACT_SHAPES:
        B, h, w = shape
        name = "%s ups %dx%dx%d" % (kind, B, h, w)
        assert hb.conv_plan(3, 24, R.EXACT_COUT, B, 2 * h, 2 * w, False, True)[0] == CONV_KINDS.index(kind)
        _check_plain(_conv_runner(hb, dev, _problem(3, R.EXACT_COUT, shape, True), B, 2 * h, 2 * w, False, True, True), name, False)
        _check_add(_conv_runner(hb, dev, _problem(3, R.EXACT_COUT_ADD, shape, True), B, 2 * h, 2 * w, False, True, True), name)
    p = R.exact_problem(3, 256, 0, 128, 2, 11, 11, True, False, "wino", 2)
    _check_plain(_conv_runner(hb, dev, p, 2, 22, 22, False, True), "%s ups deep" % kind, False)


def test_direct_split_k_exact(dev):
    """ssm_conv2d_splitk_fwd + ssm_splitk_finish_fwd on the bottleneck map (odd width: no Winograd form), with and without the addend."""
    import ctypes
    from ssm_amd import hipbind as hb
    cin, cout, B, H, W = 512, 128, 2, 11, 11
    p = R.exact_problem(3, cin, 0, cout, B, H, W, False, False, "wino")
    ks = ctypes.c_int(1)
    hb.check(hb.load().ssm_conv_splitk_plan(3, cin, cout, B, H, W, ctypes.byref(ks)))
    assert ks.value > 1
    r = _conv_runner(hb, dev, p, B, H, W, False)
    r.pk.split_ok = True
    _check_plain(r, "direct split-K", False)
    assert "_splitk_part" in r.pk.__dict__, "the split path was not taken"
    _check_add(r, "direct split-K")


def test_direct_negative_control(dev):
    from ssm_amd import hipbind as hb
    B, H, W = 2, 22, 44
    _negative_control(_conv_runner(hb, dev, _problem(3, R.EXACT_COUT, (B, H, W)), B, H, W, False), "ssm_conv.hip")


@pytest.mark.parametrize("form", ["1", "0"], ids=["valu", "mfma4x4"])
@pytest.mark.parametrize("nc", R.FINAL_NC)
def test_final_conv_both_forms_exact(dev, nc, form, monkeypatch):
    from ssm_amd import hipbind as hb
    monkeypatch.setenv("SSM_FINAL_VALU", form)
    nv = hb.NULL_VIEW
    for B, H, W in R.FINAL_SHAPES:
        p = R.exact_problem(3, 32, 0, nc, B, H, W, False, False, "direct", 3, False)
        px = hb.Planes(B, 32, H, W, dev).load(p["x"].to(dev))
        y = hb.Planes(B, nc, H, W, dev)
        wd, bd = p["w"].to(dev), p["bias"].to(dev)
        hb.check(hb.load().ssm_final_conv_fwd(px.view(), wd.data_ptr(), bd.data_ptr(), nc, y.view(), nv, nv, None, nv, nv, B, H, W,
                                              hb.stream_ptr()))
        got = y.to_nchw().cpu()
        assert torch.equal(got, p["z"]), "final_conv NC=%d %dx%dx%d: %d outputs differ" % (nc, B, H, W, int((got != p["z"]).sum()))
        assert _frame_is_zero(hb, y, H, W)


# ---- csrc/ssm_wino.hip ---------------------------------------------------------------------------------------------------------------
def _wino_runner(hb, dev, p, B, H, W, ups=False, bcast=False):
    def pack(w, b):
        return hb.PackedWino(w, b, B, H, W, ups=ups)

    def launch(av, c1, bv, c2, pk, y, yp, **kw):
        if ups:
            return hb.conv2d_ups_wino(av, c1, bv, c2, pk, y, B, H, W, **kw)
        return hb.conv2d_wino(av, c1, bv, c2, pk, y, yp, B, H, W, **kw)
    return Runner(hb, dev, p, pack, launch, bcast)


@pytest.mark.parametrize("kind", WINO_KINDS)
def test_wino_every_kind_exact(dev, kind):
    from ssm_amd import hipbind as hb
    _force(hb.load().ssm_wino_force_kind, WINO_KINDS, kind)
    for shape in R.EXACT_SHAPES:
        B, H, W = shape
        name = "%s %dx%dx%d" % (kind, B, H, W)
        assert hb.wino_plan(24, R.EXACT_COUT, B, H, W)[0] == WINO_KINDS.index(kind)
        r = _wino_runner(hb, dev, _problem(3, R.EXACT_COUT, shape), B, H, W)
        _check_plain(r, name, True, nchw_ok=W % 2 == 0, mask=True)
        _check_add(r, name)
    cin, cout, B, H, W = 64, 128, 1, 46, 80          # not split: the k-loop's double buffer over 8 chunks, several workgroup tiles
    p = R.exact_problem(3, cin, 0, cout, B, H, W, False, False, "wino", 3, False)
    r = _wino_runner(hb, dev, p, B, H, W)
    assert hb.wino_splitk(r.pk, B, H, W) == 1
    _check_plain(r, "%s deep" % kind, True)


@pytest.mark.parametrize("kind", WINO_KINDS)
def test_wino_every_kind_fused_upsample_exact(dev, kind):
    from ssm_amd import hipbind as hb
    _force(hb.load().ssm_wino_force_kind, WINO_KINDS, kind)
    for shape in R.EXACT_SHAPES:
        B, h, w = shape
        name = "%s ups %dx%dx%d" % (kind, B, h, w)
        assert hb.wino_plan(24, R.EXACT_COUT, B, 2 * h, 2 * w, True)[0] == WINO_KINDS.index(kind)
        r = _wino_runner(hb, dev, _problem(3, R.EXACT_COUT, shape, True), B, 2 * h, 2 * w, True, True)
        _check_plain(r, name, False)
        _check_add(r, name)


def test_wino_split_k_and_deep_exact(dev):
    """512 -> 128 at 2 x 22 x 22 runs split over the input channels (ssm_wino_conv2d_splitk_fwd + ssm_splitk_finish_fwd); the fused upsample
    of 256 channels at 2 x 11 x 11 low-res."""
    from ssm_amd import hipbind as hb
    cin, cout, B, H, W = R.DEEP_CASES[3]
    p = R.exact_problem(3, cin, 0, cout, B, H, W, False, False, "wino")
    r = _wino_runner(hb, dev, p, B, H, W)
    assert hb.wino_splitk(r.pk, B, H, W) > 1, "512 -> 128 at 22 x 22, batch 2: the plan does not split"
    _check_plain(r, "wino split-K", True, mask=True)
    _check_add(r, "wino split-K")
    p = R.exact_problem(3, 256, 0, 128, 2, 11, 11, True, False, "wino", 2)
    r = _wino_runner(hb, dev, p, 2, 22, 22, True)
    print("[fwd_exact] wino fused upsample 256 -> 128: KS = %d" % hb.wino_splitk(r.pk, 2, 22, 22, True))
    _check_plain(r, "wino ups deep", False)
    _check_add(r, "wino ups deep")


def test_wino_negative_control(dev):
    from ssm_amd import hipbind as hb
    B, H, W = 2, 22, 44
    _negative_control(_wino_runner(hb, dev, _problem(3, R.EXACT_COUT, (B, H, W)), B, H, W), "ssm_wino.hip")


# ---- csrc/ssm_upgemm.hip -------------------------------------------------------------------------------------------------------------
def _upgemm_runner(hb, dev, p, B, H, W, bcast):
    def pack(w, b):
        return hb.PackedUpGemm(w, b, B, H, W)

    def launch(av, c1, bv, c2, pk, y, yp, **kw):
        return hb.conv2d_ups_upgemm(av, c1, bv, c2, pk, y, B, H, W, **kw)
    return Runner(hb, dev, p, pack, launch, bcast)


@pytest.mark.parametrize("kind", UPGEMM_KINDS)
def test_upgemm_every_kind_exact(dev, kind):
    """Cout must be a multiple of 32 here: the 128-output problems of the case table serve every run."""
    from ssm_amd import hipbind as hb
    _force(hb.load().ssm_upgemm_force_kind, UPGEMM_KINDS, kind)
    for shape in R.EXACT_SHAPES:
        B, h, w = shape
        name = "%s %dx%dx%d" % (kind, B, h, w)
        r = _upgemm_runner(hb, dev, _problem(3, R.EXACT_COUT_ADD, shape, True), B, 2 * h, 2 * w, True)
        _check_plain(r, name, False, nchw_ok=(2 * w) % 4 == 0)
        _check_add(r, name)
    p = R.exact_problem(3, 256, 0, 128, 2, 11, 11, True, False, "wino", 2)
    _check_plain(_upgemm_runner(hb, dev, p, 2, 22, 22, False), "%s deep" % kind, False, nchw_ok=False)          # 22: no multiple of 4


def test_upgemm_negative_control(dev):
    from ssm_amd import hipbind as hb
    B, h, w = 2, 22, 44
    _negative_control(_upgemm_runner(hb, dev, _problem(3, R.EXACT_COUT_ADD, (B, h, w), True), B, 2 * h, 2 * w, True), "ssm_upgemm.hip")
