"""CPU checks of tests/conv_refs.py - the references that tests/test_hip_conv_fwd_exact.py and tests/test_hip_conv_fwd_oneterm.py hold the
fp32 forward convolution kernels to.  No GPU: what is proven here is that the references are what they claim to be.

  - the exactness budget passes for every case of the bit-equality module and trips on an oversized case;
  - on such operands an fp32 direct convolution gives the same bits in two channel orders (the property the bit tests rest on);
  - the sparse problems deliver at most one product per output;
  - every Winograd emulation reproduces the direct convolution in float64 (the algebra: points, scalings, block offsets) and stays
    within the error its kernel documents in fp32;
  - an emulation with ONE chosen filter-transform constant off by 1e-5 relative exceeds the one-term bar of its form (4 x the unperturbed
    emulation's own error on the same operands) - a typo the 5e-5 bar of the parity tests cannot see.  The bar does not see EVERY
    constant: a sweep over all of them counts, per form, how many it sees (all 14 of F(4x4,3x3), 9 of 32 of F(4x4,5x5), see SWEEP).
"""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_refs as R  # noqa: E402
from oracle import ssm_oracle as O  # noqa: E402


@pytest.mark.parametrize("case", R.exact_case_table(), ids=lambda c: "k%d_%d+%dto%d_%dx%dx%d%s" % (c[:7] + ("_ups" if c[7] else "",)))
def test_budget_passes_for_every_exact_case(case):
    p = R.exact_problem(*case)
    assert p["budget"] < R.TWO24
    assert float(p["z_pos"].min()) >= 0 and p["lift"] == round(p["lift"])
    k, c1, c2, cout, B = case[:5]
    if len(case) < 12:
        assert 1 in p["z_add"] and (3 in p["z_add"]) == (B % 3 == 0)


def test_some_case_serves_add_div_3():
    assert any(c[4] % 3 == 0 for c in R.exact_case_table() if len(c) < 12)


def test_budget_trips_on_an_oversized_case():
    g = torch.Generator().manual_seed(1)
    x, w, b = R.int_tensor((1, 512, 8, 8), g, -200, 200), R.int_tensor((8, 512, 3, 3), g, -200, 200), R.int_tensor((8,), g)
    with pytest.raises(AssertionError, match="leaves the exact regime"):
        R.conv_fwd_exact(x, w, b)
    # the fused upsample costs 16 x, F(2x2,3x3) a further 4 x and its own absolute sums: a case the direct form holds, the others do not
    x, w = R.int_tensor((1, 512, 8, 8), g, -80, 80), R.int_tensor((8, 512, 3, 3), g, -80, 80)
    R.conv_fwd_exact(x, w, b)
    for kw in ({"ups": True}, {"form": "wino"}):
        with pytest.raises(AssertionError, match="leaves the exact regime"):
            R.conv_fwd_exact(x, w, b, **kw)
    assert R.exactness_budget(x, w, b, form="wino") >= 4 * R.exactness_budget(x, w, b)
    with pytest.raises(AssertionError, match="integer-valued"):
        R.conv_fwd_exact(x + 0.5, w, b)


@pytest.mark.parametrize("k", [3, 5, 7])
def test_two_channel_orders_give_identical_bits_on_exact_operands(k):
    cin, cout, B, H, W = R.DEEP_CASES[k]
    p = R.exact_problem(k, cin, 0, cout, B, H, W, False, False, "wino" if k == 3 else "direct")
    fwd = R.conv2d_f32_channel_order(p["x"], p["w"], p["bias"], range(cin))
    g = torch.Generator().manual_seed(k)
    shuffled = R.conv2d_f32_channel_order(p["x"], p["w"], p["bias"], torch.randperm(cin, generator=g).tolist())
    assert torch.equal(fwd, shuffled) and torch.equal(fwd, p["z"])
    # ... and they do NOT on randn operands: the property belongs to the regime, not to the code
    xr, wr = torch.randn(1, 64, 9, 9, generator=g), torch.randn(8, 64, k, k, generator=g)
    a = R.conv2d_f32_channel_order(xr, wr, torch.zeros(8), range(64))
    b = R.conv2d_f32_channel_order(xr, wr, torch.zeros(8), reversed(range(64)))
    assert not torch.equal(a, b)


def test_lrelu_once_and_pool_bound():
    z = torch.tensor([-3.0, -0.0625, 0.0, 7.0, -1263.0])
    want = torch.tensor([-3.0 * 0.1, -0.0625 * 0.1, 0.0, 7.0, -1263.0 * 0.1], dtype=torch.float64)
    got = R.lrelu_once(z)
    assert got.dtype == torch.float32 and float((got.double() - want).abs().max()) < 2e-5
    assert torch.equal(got, torch.where(z >= 0, z, z * torch.tensor(0.1)))
    y = torch.tensor([[[[1.0, -2.0], [4.0, 8.0]]]])
    assert float(R.pool_bound(y)) == 4 * 2.0 ** -24 * 15.0


# ---- one term per output ---------------------------------------------------------------------------------------------------------------
ONETERM_CPU = [(3, 20, 32, 2, 40, 72, 5), (3, 4, 32, 1, 6, 9, 5), (5, 12, 32, 2, 40, 72, 7), (7, 9, 32, 2, 40, 72, 9), (7, 1, 32, 1, 6, 9, 9)]


@pytest.mark.parametrize("k,cin,cout,B,H,W,period", ONETERM_CPU)
def test_sparse_problem_delivers_at_most_one_term(k, cin, cout, B, H, W, period):
    x, w, bias, truth = R.sparse_problem(k, cin, cout, B, H, W, period, seed=k + cin)
    t = R.terms_per_output(x, k)
    assert float(t.max()) == 1.0 and float(t.min()) == 0.0
    assert float((x != 0).sum(1).max()) == 1.0          # one channel per lattice pixel
    nz = x[x != 0]
    assert set(nz.abs().tolist()) <= {1.0, 2.0, 4.0}
    if nz.numel() >= 6 * cin:
        assert bool((x != 0).flatten(2).any(2).any(0).all()), "every input channel occurs"
        assert set(nz.tolist()) == set(R.AMPLITUDES)
    # the truth is one product: at every output that a lattice pixel reaches, amplitude x tap + bias
    b, c, yy, xx = [int(v[0]) for v in torch.nonzero(x, as_tuple=True)]
    pad = (k - 1) // 2
    for dy in range(-pad, pad + 1):
        for dx in range(-pad, pad + 1):
            if 0 <= yy + dy < H and 0 <= xx + dx < W:
                want = x[b, c, yy, xx].double() * w[:, c, pad - dy, pad - dx].double() + bias.double()
                assert torch.equal(truth[b, :, yy + dy, xx + dx], want)
    if period > pad + 1:
        assert bool((truth[t.expand_as(truth) == 0] == bias.double().view(1, -1, 1, 1).expand_as(truth)[t.expand_as(truth) == 0]).all())


@pytest.mark.parametrize("cin,B,h,w", [(20, 2, 20, 36), (4, 1, 3, 5), (12, 1, 32, 64)])
def test_sparse_problem_under_the_fused_upsample_has_one_source_per_output(cin, B, h, w):
    """LOW-res lattice of period 5: every output of conv3x3(upsample2x(x)) is fed by at most one low-res pixel of one channel."""
    x, wt, bias, truth = R.sparse_problem(3, cin, 32, B, h, w, 5, seed=51 + cin, ups=True)
    assert tuple(truth.shape) == (B, 32, 2 * h, 2 * w)
    s = R.sources_per_output_ups(x, 3)
    assert tuple(s.shape) == (B, 1, 2 * h, 2 * w) and float(s.max()) == 1.0
    # sources_per_output_ups against the operation itself: one entry at a time, where does it reach?
    reach = torch.zeros_like(s)
    for b, c, yy, xx in torch.nonzero(x).tolist():
        one = torch.zeros(1, 1, h, w, dtype=torch.float64)
        one[0, 0, yy, xx] = 1.0
        reach[b] += (O.conv2d(O.upsample2x_bilinear(one), torch.ones(1, 1, 3, 3, dtype=torch.float64), torch.zeros(1, dtype=torch.float64)) > 0)[0]
    assert torch.equal(reach, s)
    xu = O.upsample2x_bilinear(x)          # amplitudes 1, 2, 4 times 1/16, 3/16, 9/16: fp32 holds the upsampled operand exactly
    assert xu.dtype == torch.float32 and torch.equal(xu.double(), O.upsample2x_bilinear(x.double()))
    assert torch.equal(truth, O.conv2d(xu.double(), wt.double(), bias.double()))
    if cin > 4:
        assert bool((x != 0).flatten(2).any(2).any(0).all()), "every input channel occurs"
    with pytest.raises(AssertionError):
        R.sparse_problem(3, cin, 32, B, h, w, 2, seed=1, ups=True)


# ---- the emulations --------------------------------------------------------------------------------------------------------------------
# form, k, channels, rms and max error from float64 at unit output scale AS THE KERNELS' HEADER COMMENTS DOCUMENT THEM, at the channel count
# they name:  F(4x4,3x3), 512 channels: 1.4e-6 / 1.1e-5 (csrc/ssm_wino4.hip, lines 11-13);  F(4x4,5x5), 64 channels: 3.2e-6 / 2.8e-5, and "the
# 1-D form" F(4,5) beside it: 1.4e-6 / 1.1e-5 (csrc/ssm_wino5.hip, lines 10-11);  blocked 7x7, 32 channels: 2.6e-6 / 2.9e-5, and F(2,7) in the
# same sentence: 1.0e-6 / 6.7e-6 (csrc/ssm_wino7.hip, lines 19-20).
DOCUMENTED = [("wino4", 3, 512, 1.4e-6, 1.1e-5), ("wino5", 5, 64, 3.2e-6, 2.8e-5), ("wino7", 7, 32, 2.6e-6, 2.9e-5),
              ("wino1d", 7, 32, 1.0e-6, 6.7e-6), ("wino1d", 5, 64, 1.4e-6, 1.1e-5)]
DOC_SAMPLE = 1.25          # the documented figures come from other operands of the same distribution


def _random_problem(k, cin, cout=32, B=1, H=18, W=27, seed=0):
    g = torch.Generator().manual_seed(seed + k)
    x = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    bias = torch.randn(cout, generator=g) * 0.1
    return x, w, bias, O.conv2d(x.double(), w.double(), bias.double())


@pytest.mark.parametrize("form,k,cin,doc_rms,doc_max", DOCUMENTED)
def test_emulation_is_the_convolution_in_float64_and_within_the_documented_error_in_fp32(form, k, cin, doc_rms, doc_max):
    x, w, bias, truth = _random_problem(k, cin)          # 18 x 27: ragged for every tile
    alg = R.EMULATIONS[form](x, w, bias, torch.float64)
    assert float((alg - truth).abs().max()) < 1e-11, "the Cook-Toom matrices do not reproduce the convolution"
    emax, erms = R.emulation_error(form, x, w, bias, truth)
    print("[conv_refs] %s k%d cin %d: emulation rms %.2e max %.2e (documented %.1e / %.1e)" % (form, k, cin, erms, emax, doc_rms, doc_max))
    assert erms <= doc_rms * DOC_SAMPLE and emax <= doc_max * DOC_SAMPLE
    assert erms > 1e-7, "an fp32 Winograd form cannot be as good as that: is the emulation running in float64?"


def test_f23_is_exact_on_integer_operands():
    """F(2x2,3x3) with the kernel's matrices in fp32 == the exact reference, bit for bit, on a case inside the budget."""
    p = R.exact_problem(3, 16, 8, 40, 2, 22, 44, False, False, "wino")
    AT, G, BT = R.f23_matrices()
    got = R.winograd_2d(p["x"], p["w"], p["bias"], AT, G, BT, 2, 3, torch.float32)
    assert torch.equal(got, p["z"])


def test_documented_scalings_make_b_transposed_monic():
    """'the scaling that goes with the monic rows of B^T in the kernel' (csrc/ssm_wino7_pack.h): the documented c ARE that scaling."""
    for form in ("wino7", "wino4"):
        BT = R.form_matrices(form)[4]
        for row in BT:
            assert abs(float(row[row.abs() > 1e-12][-1]) - 1.0) < 1e-12
    _, G7, _ = R.cook_toom(4, 4, R.PTS_7)          # monic by construction == the documented constants
    assert float((G7 - R.form_matrices("wino7")[3]).abs().max()) < 1e-14


# The entries below are CHOSEN: constants whose 1e-5 change the bar sees.  It does not see every constant - the sweep after it counts them.
PERTURB = [("wino4", 3, 20, 5, (1, 2)), ("wino4", 3, 20, 5, (3, 1)), ("wino5", 5, 20, 7, (3, 4)), ("wino5", 5, 20, 7, (5, 0)),
           ("wino7", 7, 9, 9, (1, 0)), ("wino7", 7, 9, 9, (4, 3)), ("wino1d", 7, 9, 9, (2, 6)), ("wino1d", 5, 20, 7, (6, 2))]


@functools.lru_cache(maxsize=None)
def _perturb_case(form, k, cin, period):
    x, w, bias, truth = R.sparse_problem(k, cin, 32, 2, 40, 72, period, seed=7)
    return x, w, bias, truth, R.oneterm_bar(R.emulation_error(form, x, w, bias, truth)[0], truth)


@pytest.mark.parametrize("form,k,cin,period,entry", PERTURB)
def test_one_constant_off_by_1e_5_exceeds_the_oneterm_bar(form, k, cin, period, entry):
    """One chosen constant per case (the issue asks for one): off by 1e-5 relative it exceeds the one-term bar and stays under 5e-5."""
    x, w, bias, truth, bar = _perturb_case(form, k, cin, period)
    G = R.perturbed(R.filter_transform_matrix(form, k), *entry)
    emax, _ = R.emulation_error(form, x, w, bias, truth, G=G)
    print("[conv_refs] %s G[%d][%d] x (1 + 1e-5): error %.3e, bar %.3e" % (form, entry[0], entry[1], emax, bar))
    assert emax > bar, "the one-term bar does not see a constant off by 1e-5"
    assert emax < 5e-5, "... which the parity bar of 5e-5 lets through"


# form, k, cin, period, non-zero constants of G, the least number of them the bar must see.  Recorded on these operands (error of the
# perturbed emulation as a fraction of the bar in brackets): F(4x4,3x3) 14 of 14 (1.4 - 8.5); blocked 7x7 19 of 22 (0.5 - 5.3);
# F(4,5) 28 of 32 (0.8 - 22); F(2,7) 32 of 44 (0.2 - 13); F(4x4,5x5) 9 of 32 (0.26 - 2.8) - its own fp32 error is the largest of the forms,
# and with it the bar.  The constants it misses are the small ones: 1e-5 of G[i][j] g[j] is then a fraction of the form's rounding error,
# which no comparison with float64 can tell from it.  The minimum asserted is the recorded count less the entries within 15 % above
# the bar (another BLAS may sum them to the other side); NONE of the 144 reaches the 5e-5 parity bar.
SWEEP = [("wino4", 3, 20, 5, 14, 14), ("wino5", 5, 20, 7, 32, 6), ("wino7", 7, 9, 9, 22, 16), ("wino1d", 7, 9, 9, 44, 28),
         ("wino1d", 5, 20, 7, 32, 28)]


@pytest.mark.parametrize("form,k,cin,period,constants,least", SWEEP)
def test_how_many_constants_off_by_1e_5_the_oneterm_bar_sees(form, k, cin, period, constants, least):
    x, w, bias, truth, bar = _perturb_case(form, k, cin, period)
    G0 = R.filter_transform_matrix(form, k)
    ratio = {}
    for i, j in torch.nonzero(G0).tolist():
        ratio[(i, j)] = R.emulation_error(form, x, w, bias, truth, G=R.perturbed(G0, i, j))[0] / bar
    seen = sum(r > 1.0 for r in ratio.values())
    print("[conv_refs] %s k%d: the bar sees %d of %d constants off by 1e-5 (error / bar %.2f .. %.2f); missed: %s"
          % (form, k, seen, len(ratio), min(ratio.values()), max(ratio.values()), sorted(e for e, r in ratio.items() if r <= 1.0)))
    assert len(ratio) == constants
    assert seen >= least, "the one-term bar sees %d of %d constants, %d expected" % (seen, constants, least)
    assert max(ratio.values()) * bar < 5e-5, "the parity bar of 5e-5 lets every one of them through"


def test_packed_references_have_the_documented_layout():
    g = torch.Generator().manual_seed(3)
    w5, w7 = torch.randn(40, 7, 5, 5, generator=g), torch.randn(40, 7, 7, 7, generator=g)
    p5, p7 = R.packed_wino5_reference(w5), R.packed_wino7_reference(w7)
    assert tuple(p5.shape) == (2, 2, 16, 4, 32, 4) and tuple(p7.shape) == (2, 7, 14, 4, 32, 4)
    G5, G7 = R.form_matrices("wino5")[3], R.form_matrices("wino7")[3]
    # couts 33: block 1, n = 1; cin 6: chunk 1, cq 2; row frequency 3, column frequency 7 (quad 6, element 3) / 4 (quad 7, element 1)
    U = G5 @ w5[33, 6].double() @ G5.T
    assert float(p5[1, 1, 6, 2, 1, 3]) == float(U[3, 7]) and float(p5[1, 1, 7, 2, 1, 1]) == float(U[3, 4])
    assert float(p5[:, 1, :, 3].abs().max()) == 0.0 and float(p5[1, :, :, :, 8:].abs().max()) == 0.0          # cin 7, couts 40..63
    g8 = torch.zeros(8, 8, dtype=torch.float64)
    g8[:7, :7] = w7[33, 6].double()
    U = G7 @ g8[4:8, 0:4] @ G7.T                      # block 2: rows 4..7, columns 0..3
    assert abs(float(p7[1, 6, 2 * 5 + 1, 2, 1, 2]) - float(U[5, 6])) < 1e-15 and float(p7[:, :, 1::2, :, :, 3].abs().max()) == 0.0
    assert float(R.ulp_distance(torch.tensor([1.0 + 2.0 ** -23]), torch.tensor([1.0], dtype=torch.float64))) == 1.0
