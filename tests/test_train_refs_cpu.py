"""The float64 references of tests/train_refs.py are usable yardsticks at every shape and flow scale the GPU suite
(tests/test_hip_train_elementwise.py) runs: keep_mask drops at most 1 % of the pixels, and on the kept pixels the fp32 CPU oracle
sits within 1e-5 (relative to the largest entry) of the float64 one.  The same for the forward references and case lists of
tests/test_hip_infer_elementwise.py: the constructed flow family, the saturated synthesis case, the exact-integer cases.  No GPU."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_refs as R  # noqa: E402

CASES = R.SAMPLER_CASES + R.LOSS_ONLY_CASES
TERMS = [(1, 1), (0, 1), (1, 0), (0, 0)]


@pytest.mark.parametrize("shape,scale", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_keep_mask_and_fp32_oracle_gap(shape, scale):
    c = R.make_case(shape, scale)
    for s1, s2 in TERMS:
        for extra in (None, c["dy_extra"]):
            args = (c["img6"], c["flow4"], c["out5"], c["target"], c["t"], c["c_rec"], c["c_warp"], c["r16"], extra, s1, s2)
            hi = R.loss_and_grads(*args, dtype=torch.float64)
            lo = R.loss_and_grads(*args, dtype=torch.float32)
            keep = R.keep_mask(hi["flows"], hi["l1_args"])
            share = R.excluded_share(keep)
            gaps = [R.rel_err(lo[k], hi[k], keep) for k in ("dout5", "dflow4")]
            sums = float(((lo["sums"].double() - hi["sums"]).abs() / hi["sums"].abs().clamp_min(1e-300)).max())
            print("%s x%g terms=(%d,%d) extra=%d: excluded %.3f %%, fp32 oracle gap dout5 %.2e dflow4 %.2e sums %.2e"
                  % (shape, scale, s1, s2, extra is not None, 100 * share, gaps[0], gaps[1], sums))
            assert share <= 0.01, "keep_mask drops %.2f %% of the pixels" % (100 * share)
            assert max(gaps) <= 1e-5, gaps
            assert sums <= 1e-5, sums          # the sums are continuous: no mask


@pytest.mark.parametrize("shape,scale", R.SAMPLER_CASES, ids=lambda v: str(v).replace(" ", ""))
@pytest.mark.parametrize("C", [1, 3, 6])
def test_warp_reference_gap(shape, scale, C):
    B, H, W = shape
    g = torch.Generator().manual_seed(R.SEED + C)
    img, dy = torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g)
    flow = torch.randn(B, 2, H, W, generator=g) * scale
    keep = R.keep_mask([flow])
    assert R.excluded_share(keep) <= 0.01
    e_flow, e_img = R.ref_gap(lambda dt: R.warp_grads(img, flow, dy, dt))
    lo, hi = R.warp_grads(img, flow, dy, torch.float32), R.warp_grads(img, flow, dy, torch.float64)
    assert R.rel_err(lo[0], hi[0], keep) <= 1e-5
    assert e_img <= 1e-5                       # the scattered image gradient is continuous in the coordinates: no mask


def test_keep_mask_drops_what_it_should():
    flow = torch.zeros(1, 2, 3, 4)
    flow[0, 0, 1, 2] = 0.5          # x + u = 2.5: kept
    flow[0, 1, 1, 2] = 0.25
    keep = R.keep_mask([flow + 0.25])
    assert keep.all()
    keep = R.keep_mask([flow])       # every other pixel sits on the grid
    assert int(keep.sum()) == 1 and bool(keep[0, 1, 2])
    arg = torch.ones(1, 3, 3, 4)
    arg[0, 1, 2, 3] = 5e-6
    keep = R.keep_mask([flow + 0.25], [arg])
    assert int((~keep).sum()) == 1 and not bool(keep[0, 2, 3])
    # an axis of one pixel carries no coordinate: only the other axis is windowed
    assert R.keep_mask([torch.full((1, 2, 5, 1), 0.5)]).all()
    assert not R.keep_mask([torch.zeros(1, 2, 5, 1)]).any()


def test_cell_formulas_are_the_oracle_cells_without_their_convolutions():
    from oracle import ssm_oracle as O
    g = torch.Generator().manual_seed(5)
    B, Cx, Hc, H, W = 2, 3, 8, 5, 7
    x, h, c = (torch.randn(B, n, H, W, generator=g, dtype=torch.float64) for n in (Cx, Hc, Hc))
    w, b = torch.randn(4 * Hc, Cx + Hc, 3, 3, generator=g, dtype=torch.float64) * 0.2, torch.randn(4 * Hc, generator=g, dtype=torch.float64)
    want = O.convlstm_cell(x, h, c, w, b)
    got = R.lstm_cell(O.conv2d(torch.cat([x, h], 1), w, b), c)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    wg, bg = torch.randn(2 * Hc, Cx + Hc, 3, 3, generator=g, dtype=torch.float64) * 0.2, torch.randn(2 * Hc, generator=g, dtype=torch.float64)
    wc, bc = torch.randn(Hc, Cx + Hc, 3, 3, generator=g, dtype=torch.float64) * 0.2, torch.randn(Hc, generator=g, dtype=torch.float64)
    gates = O.conv2d(torch.cat([x, h], 1), wg, bg)
    cand = O.conv2d(torch.cat([x, R.gru_reset(gates, h)], 1), wc, bc)
    assert torch.equal(R.gru_update(gates, cand, h), O.convgru_cell(x, h, wg, bg, wc, bc))
    # zero state = the NULL-view forms of the first step
    z = torch.zeros_like(c)
    a, b2 = R.lstm_cell(gates.repeat(1, 2, 1, 1), None), R.lstm_cell(gates.repeat(1, 2, 1, 1), z)
    assert torch.equal(a[0], b2[0]) and torch.equal(a[1], b2[1])
    assert torch.equal(R.gru_update(gates, cand, None), R.gru_update(gates, cand, z))


# ---- the references of tests/test_hip_infer_elementwise.py ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.CONSTRUCTED_SHAPES, ids=lambda v: str(v).replace(" ", ""))
def test_constructed_flow_lands_on_its_positions(shape):
    """The flow family of the forward sampler test: in fp32, by the oracle's own coordinate steps, every pixel samples exactly at its
    target; every combination of the four classes occurs; each class is what it says; no tap inside -> the float64 oracle returns 0."""
    from oracle import ssm_oracle as O
    B, H, W = shape
    flow, tx, ty, cx, cy = R.constructed_flow(shape)
    assert flow.dtype == torch.float32
    for dt in (torch.float32, torch.float64):
        ix, iy = R.sampling_positions(flow, dt)
        assert torch.equal(ix, tx.to(dt)) and torch.equal(iy, ty.to(dt))
    assert len({(int(a), int(b)) for a, b in zip(cx.flatten(), cy.flatten())}) == 16
    for t, c, n in ((tx, cx, W), (ty, cy, H)):
        p = t[c == 0]
        assert bool((p == p.round()).all()) and bool(((p >= 0) & (p <= n - 1)).all())
        assert bool((t[c == 1] == n - 1).all())
        p = t[c == 2]
        assert bool((((p > -1) & (p < 0)) | ((p > n - 1) & (p < n))).all()) and bool((p < 0).any()) and bool((p > n - 1).any())
        p = t[c == 3]
        assert bool(((p <= -1) | (p >= n)).all()) and bool((p == -1).any()) and bool((p == n).any()) and bool((p < -1).any())
    img = torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(1))
    m = ((cx == 3) | (cy == 3)).unsqueeze(1).expand(B, 3, H, W)
    for dt in (torch.float32, torch.float64):
        out = R.warp_fwd(img, flow, dt)
        assert bool(torch.isfinite(out).all()) and not bool(out[m].any()) and bool(out[~m].any())
    # with exact positions and dyadic weights the fp32 oracle is within rounding of the float64 one
    assert R.ref_gap(lambda dt: R.warp_fwd(img, flow, dt)) <= R.ULP4


@pytest.mark.parametrize("shape,scale", R.SAMPLER_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_forward_references_and_the_saturated_case(shape, scale):
    """The fp32 oracle is finite on the plain and on the saturated synthesis case and sits within 1e-5 of the float64 one with no entry left
    out (a sample is continuous in its coordinate); the saturated case reaches V0 = 0 and V0 = 1 in fp32 and keeps its denominator."""
    for c in (R.make_case(shape, scale), R.saturated_case(shape, scale)):
        in16 = R.inputs_fwd(c["img6"], c["flow4"], c["t"], torch.float64).float()
        lo = R.synth_fwd(c["img6"], in16, c["out5"], c["t"], torch.float32)
        hi = R.synth_fwd(c["img6"], in16, c["out5"], c["t"], torch.float64)
        assert all(bool(torch.isfinite(z).all()) for z in lo + hi)
        gaps = [R.rel_err(a, b) for a, b in zip(lo, hi)]
        gaps.append(R.ref_gap(lambda dt: R.inputs_fwd(c["img6"], c["flow4"], c["t"], dt)))
        print("%s x%g: fp32 oracle gap y3 %.2e flows %.2e V0 %.2e in16 %.2e" % ((shape, scale) + tuple(gaps)))
        assert max(gaps) <= 1e-5, gaps
    v0, t = lo[2], c["t"].view(-1, 1, 1, 1)
    assert bool((v0 == 0).any()) and bool((v0 == 1).any())
    assert float(((1 - t) * v0 + t * (1 - v0)).min()) >= 0.125


def test_integer_cases_are_exact():
    """Every exact-arithmetic case of the GPU module: the float64 reference is representable in fp32 (exact_f32 asserts it), so the GPU
    comparison is a bit comparison; the slope-0.1 option is the one that is not."""
    from oracle import ssm_oracle as O
    for C in R.AVGPOOL_C:
        for H, W in R.AVGPOOL_HW:
            R.exact_f32(O.avg_pool2(R.avgpool_case(C, H, W).double()))
    for Ca, Cb in R.UPSAMPLE_CH:
        for h, w in R.UPSAMPLE_HW:
            for bcast in (False, True):
                a, b, cat = R.upsample_case(Ca, Cb, h, w, bcast=bcast)
                assert cat.shape == (2, Ca + Cb, h, w)
                R.exact_f32(O.upsample2x_bilinear(cat.double()))
    inexact = 0
    for KS in R.FINISH_KS:
        for C in R.FINISH_C:
            for H, W in R.FINISH_HW:
                d = R.finish_case(KS, C, H, W)
                for name, div, lrelu, mask, pool, slope in R.FINISH_OPTIONS:
                    if pool and (H % 2 or W % 2):
                        continue
                    y, p = R.splitk_finish_ref(d["part"], KS, add=d[div] if div else None, add_div=max(div, 1), slope=slope, lrelu=lrelu,
                                               mask=mask, pool=pool)
                    assert y.shape == (2, C, H, W) and (p is None) == (not pool)
                    if slope == R.FINISH_SLOPE:
                        R.exact_f32(y)
                        if pool:
                            R.exact_f32(p)
                    else:
                        inexact += not bool((y.float().double() == y).all())
    assert inexact > 0
    # the formula against a hand-worked pixel: partials 1, -3 and 2, addend -2, slope 1/8 -> -2 -> -0.25; as a mask: 0 * ... and (0 > 0 ? 1 : 1/8)
    part = torch.tensor([1.0, -3.0, 2.0]).view(3, 1, 1, 1)
    add = torch.tensor([-2.0]).view(1, 1, 1, 1)
    assert float(R.splitk_finish_ref(part, 3, add=add, lrelu=True)[0]) == -0.25
    assert float(R.splitk_finish_ref(part + 1, 3, add=add, mask=True)[0]) == 0.375
