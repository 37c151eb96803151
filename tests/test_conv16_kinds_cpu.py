"""No GPU: the case table of tests/test_hip_conv16_kinds.py reaches every tile kind in every mode (through ssm_conv16_plan, which reads
nothing but its arguments), its exact-integer references stay in the exact regime, the exact check sees a one-tap fault that the random
check at mode fast's bar cannot, and the representation-error bounds tests/test_hip_hl8_layout.py adds to its bars hold on the host model
of the two encodings."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hl8_refs as L  # noqa: E402

F64 = torch.float64


@pytest.fixture(scope="module")
def hb():
    from ssm_amd import hipbind
    hipbind.load()
    return hipbind


def _plan(hb, c, mode):
    return hb.conv16_plan(c.k, c.cin, c.cout_for(mode), c.W, ups=c.ups, q8=mode == "q8", fast=mode == "fast")


@pytest.mark.parametrize("mode", L.MODES)
def test_case_table_reaches_every_kind_in_every_mode(hb, mode):
    seen = {False: set(), True: set()}
    for c in L.ALL_CASES:
        kind, bn, kys = _plan(hb, c, mode)
        assert kind == c.kind, "%s is routed to %s" % (c.id, kind)
        assert bn == L.TILE[kind][0], (c.id, bn)
        seen[c.ups].add(kind)
    assert seen[False] == set(L.PLAIN_KINDS) and seen[True] == set(L.UPS_KINDS)
    tags = {(c.kind, c.tag[0]) for c in L.ALL_CASES}
    assert all((k, t) in tags for k in L.PLAIN_KINDS + L.UPS_KINDS for t in "abcde"), "a kind lacks one of the case families (a)..(e)"


def test_plan_reports_the_config_calls_and_refuses_what_the_kernels_refuse(hb):
    import ctypes
    lib = hb.load()
    bn, kys = ctypes.c_int(0), ctypes.c_int(0)
    for k, cout, W in ((7, 32, 64), (5, 64, 40), (3, 32, 64), (3, 64, 70), (3, 128, 64), (3, 128, 70), (3, 512, 40), (3, 5, 128)):
        for q8, fn in ((False, lib.ssm_conv16_config), (True, lib.ssm_conv16q_config)):
            hb.check(fn(k, cout, W, ctypes.byref(bn), ctypes.byref(kys)))
            for cin in (16, 128):
                assert hb.conv16_plan(k, cin, cout, W, q8=q8)[1:] == (bn.value, kys.value)
        if k == 3:
            for q8, fn in ((False, lib.ssm_conv16_ups_config), (True, lib.ssm_conv16q_ups_config)):
                hb.check(fn(cout, W, ctypes.byref(bn), ctypes.byref(kys)))
                assert hb.conv16_plan(3, 32, cout, W, ups=True, q8=q8)[1:] == (bn.value, kys.value)
    # the deep kinds differ from their shallow twins in the tile only: same packing
    assert hb.conv16_plan(3, 128, 32, 64)[0] == "H3N32D" and hb.conv16_plan(3, 112, 32, 64)[0] == "H3N32"
    assert hb.conv16_plan(3, 128, 256, 48)[0] == "H3N32W" and hb.conv16_plan(3, 112, 256, 48)[0] == "H3N32V"
    assert hb.conv16_plan(3, 64, 128, 96)[0] == "H3N128S" and hb.conv16_plan(3, 64, 128, 97)[0] == "H3N128"
    for bad in ((4, 16, 32, 64, False), (5, 16, 32, 64, True), (3, 0, 32, 64, False)):
        with pytest.raises(RuntimeError):
            hb.conv16_plan(*bad[:4], ups=bad[4])


@pytest.mark.parametrize("mode", L.MODES)
def test_exact_references_stay_below_2048(mode):
    """Every output of every exact-integer problem is an integer (slope 0.5: a half-integer) below 2048 - fp16 holds it exactly - and
    the worst-case sum of |products| times the filter pre-scale 8 stays below 2^24, so every fp32 partial sum is exact in any order."""
    for c in L.ALL_CASES:
        a, b, cat, w, bias = L.exact_inputs(c, mode)
        assert set(w.unique().tolist()) <= {-1.0, 0.0, 1.0} and float(w.abs().max()) == 1.0          # PackedConv16 picks scale 8
        x = L.upsample2x_f64(cat) if c.ups else cat.double()
        assert torch.equal(x, x.round()) and float(x.abs().max()) <= (16 if c.ups else 1)
        assert c.k * c.k * c.cin * float(x.abs().max()) * 8 + 8 * 3 < 2 ** 24
        for lrelu in ((False, True) if c.slope_half else (False,)):
            y, pool, premax = L.conv_exact(c, cat, w, bias, lrelu=lrelu)
            assert premax < 2048, (c.id, premax)
            assert torch.equal(y * 2, (y * 2).round()) and torch.equal(y.float().half().double(), y), c.id
            if pool is not None:
                assert torch.equal(pool.float().double(), pool)


def test_one_dropped_tap_exact_check_against_the_fast_bar():
    """The reason for the exact-integer check.  Cin = 144, 3x3: drop one tap of one input channel of one output channel.
    Exact data: the output changes by exactly |x| = 1 wherever that tap meets a nonzero activation - for EVERY nonzero tap.
    randn data at the oracle's filter scale 1 / sqrt(9 Cin): the output changes by |w_tap| |x|; against mode fast's bar 2e-2 the fault is
    invisible for every tap with |w_tap| max|x| < 2e-2 (and 2e-2 leaves room above the mode's own error of ~1e-3 for more)."""
    c = next(c for c in L.PLAIN_CASES if c.kind == "H3N32W" and c.tag == "d-cin144")
    a, b, cat, w, bias = L.exact_inputs(c, "fast")
    want = L.conv_exact(c, cat, w, bias)[0]
    nz = (w[0] != 0).nonzero()
    caught = 0
    for ci, ky, kx in nz.tolist():
        w2 = w.clone()
        w2[0, ci, ky, kx] = 0
        d = (L.conv_exact(c, cat, w2, bias)[0] - want).abs()
        assert float(d.max()) in (0.0, 1.0)
        caught += float(d.max()) == 1.0
    print("exact data: %d of %d nonzero taps of output channel 0 change an output by exactly 1 when dropped" % (caught, len(nz)))
    assert caught >= len(nz) - 2          # a tap is invisible only where its whole shifted activation plane is zero (tiny maps)
    a, b, cat, w, bias = L.random_inputs(c, "fast")
    y = L.conv_exact(c, cat, w, bias)[0]
    hidden, worst = 0, 0.0
    for ci in range(c.cin):
        for ky in range(3):
            for kx in range(3):
                w2 = w.clone()
                w2[0, ci, ky, kx] = 0
                d = float((L.conv_exact(c, cat, w2, bias)[0] - y).abs().max())
                hidden += d < L.BARS["fast"]
                worst = max(worst, d)
    print("randn data: %d of %d dropped taps change no output by 2e-2 (largest change of any tap %.3f)" % (hidden, 9 * c.cin, worst))
    assert hidden > 0


@pytest.mark.parametrize("q8", [False, True], ids=["hl8", "q8"])
def test_representation_error_bound_of_the_encodings(q8):
    """hl8_refs.rep_error_bound (derivation in its docstring) against the host model of the encodings, on values up to each magnitude -
    tests/test_hip_hl8_layout.py adds this bound to the fp32 siblings' bars, so it must come from the formats, not from a kernel."""
    g = torch.Generator().manual_seed(3)
    for amax in (2.0 ** -6, 0.1, 1.0, 5.0, 100.0, 447.0, 600.0, 1e4):
        x = (torch.rand(20000, generator=g) * 2 - 1) * amax
        x[0], x[1] = amax, -amax
        if q8:
            dec = L.q8_model(x)
        else:
            hi, lo = L.split_hl(x)
            dec = hi.double() + lo.double()
        err = float((dec - x.double()).abs().max())
        print("|x| <= %-8g %s: largest error %.3e  bound %.3e" % (amax, "Q8" if q8 else "HL8", err, L.rep_error_bound(amax, q8)))
        assert err <= L.rep_error_bound(amax, q8)
    # the encoder's table: every code decodes to itself, ties go to the even code, the clamp saturates
    codes = torch.arange(256, dtype=torch.uint8)
    ok = ~torch.isnan(L.E4M3)
    assert torch.equal(L.e4m3_encode(L.E4M3[ok])[1:], codes[ok][1:])
    assert L.e4m3_encode(torch.tensor([17.0, 19.0, 1e9, -1e9, 2.0 ** -10])).tolist() == [0x58, 0x5a, 0x7e, 0xfe, 0x00]
