"""The float64 references of tests/train_refs.py are usable yardsticks at every shape and flow scale the GPU suite
(tests/test_hip_train_elementwise.py) runs: keep_mask drops at most 1 % of the pixels, and on the kept pixels the fp32 CPU oracle
sits within 1e-5 (relative to the largest entry) of the float64 one.  No GPU."""
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
