"""The fp32 forward convolution forms that CANNOT be exact (non-dyadic transform constants) - csrc/ssm_wino4.hip F(4x4,3x3),
csrc/ssm_wino5.hip F(4x4,5x5), csrc/ssm_wino7.hip 2x2 blocks of F(4x4,4x4), csrc/ssm_wino1d.hip F(2,7) / F(4,5) along x - on problems in
which every output receives AT MOST ONE product (conv_refs.sparse_problem): the float64 truth is amplitude x tap + bias with no
summation, so whatever error shows is the form's own - a transform constant, a tap of one tile position fed from the wrong register -
with no 4608-term sum to hide in.

The bar is not typed in.  Per case it is conv_refs.ONETERM_MARGIN = 4 x the largest error of the form's fp32 emulation (conv_refs, built
from the documented Cook-Toom points and scalings, U in float64 rounded once, everything after it fp32; it shares no code with the
kernels) on the very same operands.  The margin covers the kernels' freedom in summation order over the 36 - 64 frequencies and FMA
contraction.  On the map smaller than a tile the emulation's largest error is one or two roundings of one output, and could by luck be
none: the bar is floored at 4 roundings (4 x 2^-24) of the largest |truth| (conv_refs.oneterm_bar) - 2.4e-7 at unit scale, below 4 x the
emulation in every case of the several-tile maps.  tests/test_conv_refs_cpu.py shows on the CPU that a chosen filter-transform constant
off by 1e-5 relative exceeds this bar, and counts how many of ALL constants do: every one of F(4x4,3x3), 19 of 22 of the blocked 7x7, 28
of 32 of F(4,5), 32 of 44 of F(2,7), 9 of 32 of F(4x4,5x5), whose own fp32 error, and with it the bar, is the largest.

Cases.  Lattice period: the smallest >= k that is coprime to 4 and to the 16 x 32 workgroup tile - 5 (3x3), 7 (5x5), 9 (7x7): over one
map every tap meets every position of the output tile and of the workgroup tile.  Maps: 2 x 40 x 72 (several workgroup tiles, ragged
edges) and 1 x 6 x 9 (smaller than a tile).  Input channels: 1..9 for the 7x7 forms, 4, 8, 12, 16, 20 for the others (the pipelines'
prologues and tails); 64 outputs.  Every tile kind of every form (6 + 2 + 4 + 5), lrelu off against the truth and lrelu on against
lrelu_once(truth in fp32); per case the max and rms error are printed, and a failure prints the max error per position inside the output tile.
Packed filters: PackedWino5.w / PackedWino7.w against a float64 U = G g G^T laid out in Python from the header comments (Cout 32 and 40, Cin 7
and 30): every entry within 1 ulp of fp32(U), padding channels and padding slots exactly zero.

F(4x4,3x3) under the fused upsample (ssm_wino4_conv2d_ups_add_fwd, all 6 kinds) and as the sub-pixel interior + border-ring pair
(ssm_wino4_conv2d_shuffle_fwd in each of its three 64-cout kinds + ssm_wino4_conv2d_ups_border_fwd): the lattice sits at LOW resolution.
A low-res pixel feeds 4 high-res pixels per axis, hence 6 outputs; with period 5 (2 x 5 >= 6) every output is fed by ONE low-res pixel of
one channel (conv_refs.sources_per_output_ups) - the float64 truth conv(up(x)) is a sum of at most 9 terms amplitude x bilinear weight x
tap.  Period 5 is odd, so the lattice pixels' high-res positions 2i take both residues 0 and 2 modulo the tile's 4, and the 4-wide
upsampled patch carries each of its weights to every tile position.  The emulation is F(4x4,3x3) of the upsampled operand, which fp32
holds exactly; the bar is 4 x its error, the same for the pair.  Maps (low-res): 2 x 20 x 36 and 1 x 3 x 5 (outputs 2 x 40 x 72 and
1 x 6 x 10); the pair on 2 x 32 x 64 -> 64 x 128, the smallest output subpixel_wino4_supported accepts, 32 outputs, the output buffer
NaN before the launches (every pixel written) and the error of the border ring printed on its own.  Input channels 4, 8, 12, 16, 20.

Not covered here: the packed layouts of PackedWino4 / PackedWino1d (not read from the pack kernels in the time this module had).

What was found (MI355X).  Every kind of every form inside its bar.  On the several-tile maps no case exceeds 1.5 x its emulation (the
largest: F(2,7) cin 8, 1.47 x = 0.37 of the bar; fused upsample 1.26 x; the pair 0.93 x); on the maps smaller than a tile, where the
emulation's largest error is one or two roundings, 2.1 x at the most (F(2,7) cin 6: 1.08e-7 | 2.28e-7, 0.53 of the bar).  The kinds of a form
agree to the last printed digit in most cases (they differ in tiling, not in arithmetic).  Largest error over the channel counts, emulated | measured
(2 x 40 x 72; the 1 x 6 x 9 map in brackets), the bar being 4 x the emulated figure of the same case:
    F(4x4,3x3)  wino4   cin  4: 2.33e-6 | 2.80e-6     cin 20: 1.66e-6 | 1.61e-6     (cin 20: 6.0e-8 | 1.1e-7)
    F(4x4,5x5)  wino5   cin  4: 1.03e-5 | 8.11e-6     cin 20: 3.96e-6 | 3.37e-6     (cin 20: 4.7e-7 | 6.0e-7)
    blocked 7x7 wino7   cin  1: 6.71e-6 | 5.82e-6     cin  4: 2.68e-6 | 2.68e-6     cin 9: 2.86e-6 | 1.58e-6     (cin 9: 1.5e-7 | 8.9e-8)
    F(2,7)      wino1d  cin  1: 1.72e-6 | 1.82e-6     cin  4: 8.05e-7 | 8.31e-7     cin 9: 6.84e-7 | 6.87e-7     (cin 9: 1.7e-7 | 8.9e-8)
    F(4,5)      wino1d  cin  4: 1.12e-6 | 1.10e-6     cin 20: 4.69e-7 | 4.84e-7     (cin 20: 1.7e-7 | 1.7e-7)
    F(4x4,3x3) fused upsample, X4A   cin 4: 1.76e-6 | 2.12e-6   cin 8: 1.29e-6 | 1.05e-6   cin 12: 1.00e-6 | 1.25e-6   cin 16: 1.41e-6 | 8.66e-7
                                     cin 20: 1.04e-6 | 7.94e-7     (1 x 6 x 10, cin 4: 4.06e-7 | 3.13e-7   cin 12: 1.37e-7 | 2.50e-7   cin 20: 2.72e-7 | 1.29e-7)
    F(4x4,3x3) sub-pixel pair, Y4A   cin 4: 1.70e-6 | 1.58e-6   cin 8: 1.25e-6 | 1.06e-6   cin 12: 1.57e-6 | 1.25e-6   cin 16: 9.74e-7 | 8.33e-7
                                     cin 20: 9.24e-7 | 7.55e-7     (the border ring alone: 1.58e-6 at cin 4, 7.55e-7 at cin 20)
rms errors of the plain forms agree within 5 % (e.g. wino5 cin 4: 1.70e-7 | 1.67e-7); under the upsample the kernels' rms is 20 - 25 % BELOW
the emulation's (cin 4: 4.61e-8 | 3.51e-8).  Packed filters: PackedWino5 (Cout 32; the class refuses Cout 40) and
PackedWino7 (Cout 32 and 40), Cin 7 and 30: every entry within 1 ulp of fp32(U) (the largest distance is exactly 1 ulp: the float64 sums of
the pack kernel and of einsum differ in order, and a few land on either side of a rounding boundary), all padding exactly zero.
"""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_refs as R  # noqa: E402

pytestmark = pytest.mark.gpu

KINDS = {"wino4": ["X4A", "X4B", "X4C", "Y4A", "Y4B", "Y4C"], "wino5": ["F5A", "F5B"], "wino7": ["Z7A", "Z7B", "Z7AS", "Z7BS"],
         "wino1d": ["R7A", "R7B", "R5A", "R5B", "R5C"]}
FORCE = {"wino4": "ssm_wino4_force_kind", "wino5": "ssm_wino5_force_kind", "wino7": "ssm_wino7_force_kind", "wino1d": "ssm_wino1d_force_kind"}
PERIOD = {3: 5, 5: 7, 7: 9}
MAPS = ((2, 40, 72), (1, 6, 9))
COUT = 64


def _k_of(form, kind):
    return {"wino4": 3, "wino5": 5, "wino7": 7}.get(form) or (7 if kind.startswith("R7") else 5)


def _channels(k):
    return tuple(range(1, 10)) if k == 7 else (4, 8, 12, 16, 20)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _unforce():
    yield
    from ssm_amd import hipbind as hb
    for fn in FORCE.values():
        getattr(hb.load(), fn)(-1)


def _force(form, kind):
    from ssm_amd import hipbind as hb
    n = getattr(hb.load(), FORCE[form])(KINDS[form].index(kind))
    assert n == len(KINDS[form]), "tile-configuration list of the test is out of date (%d in the library)" % n


@functools.lru_cache(maxsize=None)
def _case(form, k, cin, B, H, W):
    """Operands, float64 truth and the emulation's (max, rms) error of one case: computed once, shared by the kinds of a form."""
    x, w, bias, truth = R.sparse_problem(k, cin, COUT, B, H, W, PERIOD[k], seed=17 * k + cin)
    assert float(R.terms_per_output(x, k).max()) <= 1.0
    return x, w, bias, truth, R.emulation_error(form, x, w, bias, truth)


@functools.lru_cache(maxsize=None)
def _ups_case(cin, cout, B, h, w):
    """The same under the fused upsample: a LOW-res lattice, one source per output; the emulation is F(4x4,3x3) of the upsampled operand
    (which fp32 holds exactly: amplitudes 1, 2, 4 times 1/16, 3/16, 9/16)."""
    from oracle import ssm_oracle as O
    x, wt, bias, truth = R.sparse_problem(3, cin, cout, B, h, w, PERIOD[3], seed=51 + cin, ups=True)
    assert float(R.sources_per_output_ups(x, 3).max()) <= 1.0
    return x, wt, bias, truth, R.emulation_error("wino4", O.upsample2x_bilinear(x), wt, bias, truth)


def _verdict(name, truth, emu, got, act, tw=4):
    """Prints emulated and measured errors of one case; -> None, or what the failure message says (with the per-tile-position table)."""
    emax, erms = emu
    bar = R.oneterm_bar(emax, truth)
    err = got.double() - truth
    gmax, grms = float(err.abs().max()), float(err.pow(2).mean().sqrt())
    amax = float((act.double() - R.lrelu_once(truth.float()).double()).abs().max())
    print("[oneterm] %s: emulated max %.3e rms %.3e | measured max %.3e rms %.3e lrelu max %.3e | bar %.3e"
          % (name, emax, erms, gmax, grms, amax, bar))
    if gmax <= bar and amax <= bar + 2.0 ** -24 * float(truth.abs().max()):          # lrelu_once starts from the ROUNDED truth
        return None
    return "%s: measured %.3e (lrelu %.3e) > bar %.3e; per tile position:\n%s" % (name, gmax, amax, bar, R.tile_position_table(err, 4, tw))


def _launch(hb, form, dev, x, w, bias, lrelu):
    B, cin, H, W = x.shape
    cls = {"wino4": hb.PackedWino4, "wino5": hb.PackedWino5, "wino7": hb.PackedWino7, "wino1d": hb.PackedWino1d}[form]
    fn = {"wino4": hb.conv2d_wino4, "wino5": hb.conv2d_wino5, "wino7": hb.conv2d_wino7, "wino1d": hb.conv2d_wino1d}[form]
    pk = cls(w.to(dev), bias.to(dev), B, H, W)
    px = hb.Planes(B, pk.cin_p, H, W, dev)          # channels beyond cin (the form's padding) stay zero
    px.interior[:, :cin] = x.to(dev)
    y = hb.Planes(B, COUT, H, W, dev)
    fn(px.view(), pk.cin_p, None, 0, pk, y.view(), None, B, H, W, lrelu=lrelu)
    full = y.full.clone()
    full[:, :, hb.SSM_PADY:hb.SSM_PADY + H, hb.SSM_PADX:hb.SSM_PADX + W] = 0
    assert not bool(full.any()), "wrote outside the interior"
    return y.to_nchw().cpu()


ALL = [(form, kind) for form in ("wino4", "wino5", "wino7", "wino1d") for kind in KINDS[form]]


@pytest.mark.parametrize("form,kind", ALL, ids=["%s-%s" % fk for fk in ALL])
def test_one_term_per_output_within_four_times_the_emulation(dev, form, kind):
    from ssm_amd import hipbind as hb
    k = _k_of(form, kind)
    _force(form, kind)
    tw = 2 if (form == "wino1d" and k == 7) else 4
    failures = []
    for B, H, W in MAPS:
        for cin in _channels(k):
            x, w, bias, truth, emu = _case(form, k, cin, B, H, W)
            failures.append(_verdict("%s %s k%d cin %2d %dx%dx%d" % (form, kind, k, cin, B, H, W), truth, emu,
                                     _launch(hb, form, dev, x, w, bias, False), _launch(hb, form, dev, x, w, bias, True), tw))
    assert not any(failures), "\n".join(f for f in failures if f)


# ---- F(4x4,3x3) under the fused upsample, and its sub-pixel interior + border-ring pair ---------------------------------------------------
UPS_MAPS = ((2, 20, 36), (1, 3, 5))          # LOW-res (B, h, w): outputs 2 x 40 x 72 and 1 x 6 x 10
PAIR_MAP, PAIR_COUT = (2, 32, 64), 32        # LOW-res: the 64 x 128 output is the smallest map subpixel_wino4_supported accepts


def _frame_is_zero(hb, y, H, W):
    full = y.full.clone()
    full[:, :, hb.SSM_PADY:hb.SSM_PADY + H, hb.SSM_PADX:hb.SSM_PADX + W] = 0
    return not bool(full.any())


@pytest.mark.parametrize("kind", KINDS["wino4"])
def test_one_source_per_output_fused_upsample_within_four_times_the_emulation(dev, kind):
    """ssm_wino4_conv2d_ups_add_fwd, every kind: conv3x3(upsample2x(x)) of a low-res lattice against the float64 truth."""
    from ssm_amd import hipbind as hb
    _force("wino4", kind)
    failures = []
    for B, h, w in UPS_MAPS:
        H, W = 2 * h, 2 * w
        for cin in _channels(3):
            x, wt, bias, truth, emu = _ups_case(cin, COUT, B, h, w)
            pk = hb.PackedWino4(wt.to(dev), bias.to(dev), B, H, W, ups=True)
            px = hb.Planes(B, cin, h, w, dev).load(x.to(dev))
            out = []
            for lrelu in (False, True):
                y = hb.Planes(B, COUT, H, W, dev)
                hb.conv2d_ups_wino4(px.view(), cin, None, 0, pk, y.view(), B, H, W, lrelu=lrelu)
                assert _frame_is_zero(hb, y, H, W), "wrote outside the interior"
                out.append(y.to_nchw().cpu())
            failures.append(_verdict("wino4 ups %s cin %2d %dx%dx%d" % (kind, cin, B, H, W), truth, emu, *out))
    assert not any(failures), "\n".join(f for f in failures if f)


@pytest.mark.parametrize("kind", ["Y4A", "Y4B", "Y4C"])          # the interior runs in a 64-cout kind (the forced one, Y4A otherwise)
def test_one_source_per_output_subpixel_pair_within_four_times_the_emulation(dev, kind):
    """ssm_wino4_conv2d_shuffle_fwd on the interior + ssm_wino4_conv2d_ups_border_fwd on the ring of 16 x 32 tiles, against the same truth
    and the same bar as the fused-upsample kernel: every pixel written once (the output starts as NaN), the ring reported on its own."""
    from ssm_amd import hipbind as hb
    _force("wino4", kind)
    B, h, w = PAIR_MAP
    H, W = 2 * h, 2 * w
    failures = []
    for cin in _channels(3):
        assert hb.subpixel_wino4_supported(cin, PAIR_COUT, H, W)
        x, wt, bias, truth, emu = _ups_case(cin, PAIR_COUT, B, h, w)
        pk = hb.PackedSubpixelWino4(wt.to(dev), bias.to(dev), B, H, W)
        px = hb.Planes(B, cin, h, w, dev).load(x.to(dev))
        out = []
        for lrelu in (False, True):
            y = hb.Planes(B, PAIR_COUT, H, W, dev)
            y.interior.fill_(float("nan"))
            hb.conv2d_ups_subpixel_wino4(lambda y0, x0: px.view(y0=y0, x0=x0), cin, None, 0, pk, lambda y0, x0: y.view(y0=y0, x0=x0), B, H, W,
                                         lrelu=lrelu)
            got = y.to_nchw().cpu()
            assert bool(torch.isfinite(got).all()), "pixels left unwritten"
            assert _frame_is_zero(hb, y, H, W), "wrote outside the interior"
            out.append(got)
        ring = (out[0].double() - truth).abs()
        ring[:, :, hb.WINO4_BORDER_TH:H - hb.WINO4_BORDER_TH, hb.WINO4_BORDER_TW:W - hb.WINO4_BORDER_TW] = 0
        print("[oneterm] wino4 pair %s cin %2d: border ring alone max %.3e" % (kind, cin, float(ring.max())))
        failures.append(_verdict("wino4 pair %s cin %2d %dx%dx%d" % (kind, cin, B, H, W), truth, emu, *out))
    assert not any(failures), "\n".join(f for f in failures if f)


# ---- packed filters -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin", [7, 30])
@pytest.mark.parametrize("cout", [32, 40])
def test_packed_wino5_and_wino7_against_float64(dev, cout, cin):
    from ssm_amd import hipbind as hb
    g = torch.Generator().manual_seed(cout + cin)
    for k, cls, ref in ((5, hb.PackedWino5, R.packed_wino5_reference), (7, hb.PackedWino7, R.packed_wino7_reference)):
        if k == 5 and cout % 32:
            continue          # F(4x4,5x5) takes whole 32-output blocks only (hb.PackedWino5 asserts it)
        w = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
        pk = cls(w.to(dev), torch.zeros(cout, device=dev), 1, 32, 32)
        want = ref(w)
        got = pk.w.cpu()
        assert got.numel() == want.numel(), "k%d: %d packed floats, the documented layout has %d" % (k, got.numel(), want.numel())
        got = got.view(want.shape)
        d = R.ulp_distance(got, want)
        print("[oneterm] packed k%d %d -> %d: max distance from fp32(U) %.2f ulp" % (k, cin, cout, float(d[want != 0].max())))
        assert bool((got[want == 0] == 0).all()), "k%d: padding channels / slots are not exactly zero" % k
        assert float(d[want != 0].max()) <= 1.0, "k%d: an entry is more than 1 ulp from fp32(U)" % k
