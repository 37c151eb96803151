"""The host binding of the fp32 convolution forms (ssm_amd/hipbind.py: the packed-filter classes and their launchers) computes, bit for
bit, what the commit noted in tests/golden/conv_forms_digest.json computed: SHA-256 digests of the packed filter, the packed bias, the
whole output planes (zero frame included) and the pooled planes for every form at the smallest shapes at which the Python layer's
branches differ; the messages of its refusals; and one stage-1 + stage-2 inference pass with the form and packing of every layer.

    python tests/test_hip_conv_forms_digest.py --record [--commit ID]

writes the fixture (every case runs twice; two different digests and nothing is written; $SSM_CONV_FORMS_DIGEST_OUT: another path to
write to, for a checkout whose tests/golden is read-only).  The module uses only names the recorded commit has as well, so the same file
records there and compares here."""
import hashlib
import json
import os
import sys
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_forms_digest.json")


def C(id, cls, fn, cin, cout, k=3, c2=0, B=1, H=8, W=12, pool=False, ups=False, add_div=0, lrelu=True, mask=False, split=None,
      nchw=False, scratch=None, also_two_sources=False):
    """One launch.  cin: the filter's input channels (c2 of them from the second source; one source: the planes hold pk.cin_p channels,
    zeros beyond cin); H, W: the OUTPUT map; add_div > 0: an addend (the mask source with mask=True) over B / add_div entries;
    split: "direct" / "wino" - the library must propose a split factor above 1; scratch="outside": the low-res GEMM handle gets a larger
    tensor than it needs; also_two_sources: the same handle launched again with its input as two sources (digest "y_two")."""
    return dict(id=id, cls=cls, fn=fn, cin=cin, cout=cout, k=k, c2=c2, B=B, H=H, W=W, pool=pool, ups=ups, add_div=add_div, lrelu=lrelu,
                mask=mask, split=split, nchw=nchw, scratch=scratch, also_two_sources=also_two_sources)


CASES = [
    # direct form (csrc/ssm_conv.hip)
    C("direct_k3_padded_cin_and_bias", "PackedConv", "conv2d", 13, 40, B=2, H=9, W=13),
    C("direct_k5", "PackedConv", "conv2d", 6, 16, k=5, H=9, W=13),
    C("direct_k7", "PackedConv", "conv2d", 6, 32, k=7, H=9, W=13),
    C("direct_pool", "PackedConv", "conv2d", 16, 32, B=2, pool=True),
    C("direct_two_sources", "PackedConv", "conv2d", 32, 32, c2=16, B=2),
    C("direct_add_div2_b4", "PackedConv", "conv2d", 16, 32, B=4, add_div=2),
    C("direct_ups_two_sources_add", "PackedConv", "conv2d_ups", 32, 32, c2=16, B=2, ups=True, add_div=1),
    C("direct_no_lrelu_nchw", "PackedConv", "conv2d", 16, 32, B=2, H=9, W=13, lrelu=False, nchw=True),
    C("direct_splitk", "PackedConv", "conv2d", 512, 512, B=2, H=11, W=11, split="direct", also_two_sources=True),
    # F(2x2,3x3) (csrc/ssm_wino.hip)
    C("wino_pool", "PackedWino", "conv2d_wino", 16, 32, B=2, pool=True),
    C("wino_two_sources", "PackedWino", "conv2d_wino", 16, 32, c2=8, B=2, H=9, W=13),
    C("wino_ups_add", "PackedWino", "conv2d_ups_wino", 16, 32, B=2, ups=True, add_div=1),
    C("wino_mask", "PackedWino", "conv2d_wino", 16, 32, B=2, H=9, W=13, add_div=1, lrelu=False, mask=True),
    C("wino_splitk_pool", "PackedWino", "conv2d_wino", 512, 512, B=2, H=22, W=22, pool=True, split="wino"),
    C("wino_splitk_ups", "PackedWino", "conv2d_ups_wino", 512, 512, B=2, H=22, W=22, ups=True, split="wino"),
    # F(4x4,3x3) (csrc/ssm_wino4.hip)
    C("wino4_pool", "PackedWino4", "conv2d_wino4", 16, 32, B=2, pool=True),
    C("wino4_ups_add_div2", "PackedWino4", "conv2d_ups_wino4", 16, 32, B=2, ups=True, add_div=2),
    C("wino4_mask", "PackedWino4", "conv2d_wino4", 16, 32, B=2, H=9, W=13, add_div=1, lrelu=False, mask=True),
    # sub-pixel interior + border ring: the smallest shape subpixel_wino4_supported accepts
    C("subpixel_wino4_one_source", "PackedSubpixelWino4", "conv2d_ups_subpixel_wino4", 8, 32, H=64, W=128, ups=True),
    C("subpixel_wino4_two_sources", "PackedSubpixelWino4", "conv2d_ups_subpixel_wino4", 8, 32, c2=4, H=64, W=128, ups=True),
    # low-res GEMM + combine pass (csrc/ssm_upgemm.hip)
    C("upgemm_add", "PackedUpGemm", "conv2d_ups_upgemm", 8, 32, H=4, W=6, ups=True, add_div=1),
    C("upgemm_own_scratch", "PackedUpGemm", "conv2d_ups_upgemm", 16, 32, c2=8, B=2, ups=True),
    C("upgemm_outside_scratch", "PackedUpGemm", "conv2d_ups_upgemm", 16, 32, c2=8, B=2, ups=True, scratch="outside"),
    # F(2,7) / F(4,5) along x (csrc/ssm_wino1d.hip)
    C("wino1d_k7_padded_cin", "PackedWino1d", "conv2d_wino1d", 6, 32, k=7, H=9, W=13),
    C("wino1d_k5", "PackedWino1d", "conv2d_wino1d", 32, 64, k=5, H=9, W=13),
    C("wino1d_pool", "PackedWino1d", "conv2d_wino1d", 6, 32, k=7, B=2, pool=True),
    C("wino1d_add", "PackedWino1d", "conv2d_wino1d", 32, 64, k=5, B=2, add_div=1),
    # F(4x4,5x5) (csrc/ssm_wino5.hip)
    C("wino5_padded_cin_pool", "PackedWino5", "conv2d_wino5", 7, 32, k=5, B=2, pool=True),
    C("wino5_mask", "PackedWino5", "conv2d_wino5", 8, 32, k=5, H=9, W=13, add_div=1, lrelu=False, mask=True),
    # 7x7 as 2x2 blocks of F(4x4,4x4) (csrc/ssm_wino7.hip)
    C("wino7", "PackedWino7", "conv2d_wino7", 6, 32, k=7, B=2, H=9, W=13),
    C("wino7_cout16_writes_32", "PackedWino7", "conv2d_wino7", 6, 16, k=7, H=9, W=13),
]
CASE_BY_ID = {c["id"]: c for c in CASES}


def digest(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def _planes(hb, x, channels, dev):
    """x [B, c, h, w] on the host in the first c of `channels` planes (the rest stay zero)."""
    B, c, h, w = x.shape
    p = hb.Planes(B, channels, h, w, dev)
    p.interior[:, :c] = x.to(dev)
    return p


def run_case(case, dev):
    """-> {"w", "b", "y"[, "pool"][, "y_two"]}: digests of one case (inputs from a CPU generator seeded by the case's name)."""
    from ssm_amd import hipbind as hb
    c = case
    g = torch.Generator().manual_seed(zlib.crc32(c["id"].encode()))
    B, H, W, cin, cout, k = c["B"], c["H"], c["W"], c["cin"], c["cout"], c["k"]
    h, w = (H // 2, W // 2) if c["ups"] else (H, W)
    x = torch.randn(B, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    bias = torch.randn(cout, generator=g) * 0.1
    addend = torch.randn(B // c["add_div"], cout, H, W, generator=g) if c["add_div"] else None
    cls, fn = getattr(hb, c["cls"]), getattr(hb, c["fn"])
    if c["cls"] == "PackedSubpixelWino4":
        assert hb.subpixel_wino4_supported(cin, cout, H, W) and not hb.subpixel_wino4_supported(cin, cout, H - 16, W)
        pk = cls(wt.to(dev), bias.to(dev), B, H, W)
    else:
        pk = cls(wt.to(dev), bias.to(dev), B, H, W, pool=c["pool"], ups=c["ups"])
    c2 = c["c2"]
    c1 = cin - c2 if c2 else pk.cin_p
    p1 = _planes(hb, x[:, :cin - c2], c1, dev)
    p2 = _planes(hb, x[:, cin - c2:], c2, dev) if c2 else None
    cout_w = getattr(pk, "cout_p", cout)          # the channels the launch writes (the 7x7 blocked form: whole 32-channel blocks)
    ynchw = torch.zeros(B, cout, H, W, device=dev) if c["nchw"] else None
    y = None if c["nchw"] else hb.Planes(B, cout_w, H, W, dev)
    yp = hb.Planes(B, cout, H // 2, W // 2, dev) if c["pool"] else None
    pa = _planes(hb, addend, cout, dev) if addend is not None else None
    if c["id"] == "wino7_cout16_writes_32":
        assert pk.cout_p == 32 and pk.b.numel() == 32 and y.C == 32
    if c["split"] == "direct":
        pk.split_ok = True
        import ctypes
        ks = ctypes.c_int(1)
        hb.check(hb.load().ssm_conv_splitk_plan(k, cin, cout, B, H, W, ctypes.byref(ks)))
        assert ks.value > 1, "the library proposes no split for the direct form at this shape"
    if c["split"] == "wino":
        assert hb.wino_splitk(pk, B, H, W, c["ups"]) > 1, "the library proposes no split for F(2x2,3x3) at this shape"
    if c["scratch"] == "outside":
        pk.scratch = torch.empty(2 * pk.scratch_floats(B, H, W) + 64, dtype=torch.float32, device=dev)
    kw = dict(lrelu=c["lrelu"])
    if pa is not None:
        kw.update(add=pa.view(), add_div=c["add_div"])
    if c["mask"]:
        kw.update(mask=True)
    out = {}
    if c["cls"] == "PackedSubpixelWino4":
        fn(lambda y0, x0: p1.view(y0=y0, x0=x0), c1, (lambda y0, x0: p2.view(y0=y0, x0=x0)) if c2 else None, c2, pk,
           lambda y0, x0: y.view(y0=y0, x0=x0), B, H, W, **kw)
        out["inner_w"], out["inner_b"] = digest(pk.inner.w), digest(pk.inner.b)
    else:
        yv = hb.view_of(ynchw) if c["nchw"] else y.view()
        args = (p1.view(), c1, p2.view() if c2 else None, c2, pk, yv) + (() if c["ups"] else (yp.view() if yp else None,)) + (B, H, W)
        fn(*args, **kw)
    torch.cuda.synchronize()
    if c["scratch"] == "outside":
        assert pk.scratch.numel() == 2 * pk.scratch_floats(B, H, W) + 64, "a large enough scratch tensor was replaced"
    elif c["cls"] == "PackedUpGemm":
        assert pk.scratch is not None and pk.scratch.numel() == pk.scratch_floats(B, H, W)
    out.update(w=digest(pk.w), b=digest(pk.b), y=digest(ynchw if c["nchw"] else y.full))
    if yp is not None:
        out["pool"] = digest(yp.full)
    if c["also_two_sources"]:          # (a split launch offsets its first source: two sources fall through to the plain kernel)
        half = cin // 2
        q1, q2 = _planes(hb, x[:, :half], half, dev), _planes(hb, x[:, half:], cin - half, dev)
        y2 = hb.Planes(B, cout_w, H, W, dev)
        fn(q1.view(), half, q2.view(), cin - half, pk, y2.view(), None, B, H, W, **kw)
        torch.cuda.synchronize()
        out["y_two"] = digest(y2.full)
    return out


# ---- refusals: (id, function of (hb, dev) that must raise) -----------------------------------------------------------------------------
def _pk(hb, dev, cls, cin, cout, k, B=1, H=8, W=12, **kw):
    g = torch.Generator().manual_seed(cin * 1000 + cout)
    return getattr(hb, cls)(torch.randn(cout, cin, k, k, generator=g).to(dev), torch.randn(cout, generator=g).to(dev), B, H, W, **kw)


def _views(hb, dev, pk, extra=0, ups=False):
    """Input and output views of a 1 x 8 x 12 launch, large enough for it (a refusal that failed to fire must not write out of bounds)."""
    h, w = (4, 6) if ups else (8, 12)
    return hb.Planes(1, pk.cin_p + extra, h, w, dev).view(), hb.Planes(1, getattr(pk, "cout_p", pk.cout), 8, 12, dev).view()


def _wrong_channels(cls, fn, cin, cout, k, ups=False):
    def run(hb, dev):
        pk = _pk(hb, dev, cls, cin, cout, k, ups=ups)
        x, y = _views(hb, dev, pk, 8, ups)
        getattr(hb, fn)(*((x, pk.cin_p + 8, None, 0, pk, y) + (() if ups else (None,)) + (1, 8, 12)))
    return run


def _other_shape(cls, fn, plan, cin, cout, k, shape):
    """A filter packed for a 1 x 8 x 12 launch, launched at `shape` - refused only if the two plans differ, so that is asserted first (the
    launch must never start: the views are small planes)."""
    def run(hb, dev):
        pk = _pk(hb, dev, cls, cin, cout, k)
        assert plan(hb, pk, 1, 8, 12)[1:] == (pk.bn, pk.ck) != plan(hb, pk, *shape)[1:], "the two shapes share a tile configuration"
        x, y = _views(hb, dev, pk)
        getattr(hb, fn)(x, pk.cin_p, None, 0, pk, y, None, *shape)
    return run


def _other_tiles(cls, fn, cin, cout, k, ups=False):
    """The handle's cout block changed under the launcher (forms whose plan does not move with batch or size at any shape a test can hold)."""
    def run(hb, dev):
        pk = _pk(hb, dev, cls, cin, cout, k, ups=ups)
        pk.bn += 32
        x, y = _views(hb, dev, pk, 0, ups)
        getattr(hb, fn)(*((x, pk.cin_p, None, 0, pk, y) + (() if ups else (None,)) + (1, 8, 12)))
    return run


def _second_source(cls, fn, cin, cout, k):
    def run(hb, dev):
        pk = _pk(hb, dev, cls, cin, cout, k)
        x, y = _views(hb, dev, pk)
        getattr(hb, fn)(x, pk.cin_p - 4, x, 4, pk, y, None, 1, 8, 12)
    return run


REFUSALS = [
    ("channels_direct", _wrong_channels("PackedConv", "conv2d", 16, 32, 3)),
    ("channels_direct_ups", _wrong_channels("PackedConv", "conv2d_ups", 16, 32, 3, ups=True)),
    ("channels_wino", _wrong_channels("PackedWino", "conv2d_wino", 16, 32, 3)),
    ("channels_wino_ups", _wrong_channels("PackedWino", "conv2d_ups_wino", 16, 32, 3, ups=True)),
    ("channels_wino4", _wrong_channels("PackedWino4", "conv2d_wino4", 16, 32, 3)),
    ("channels_wino4_ups", _wrong_channels("PackedWino4", "conv2d_ups_wino4", 16, 32, 3, ups=True)),
    ("channels_upgemm", _wrong_channels("PackedUpGemm", "conv2d_ups_upgemm", 16, 32, 3, ups=True)),
    ("channels_wino1d", _wrong_channels("PackedWino1d", "conv2d_wino1d", 6, 32, 7)),
    ("channels_wino5", _wrong_channels("PackedWino5", "conv2d_wino5", 8, 32, 5)),
    ("channels_wino7", _wrong_channels("PackedWino7", "conv2d_wino7", 6, 32, 7)),
    ("plan_direct", _other_shape("PackedConv", "conv2d", lambda hb, pk, B, H, W: hb.conv_plan(3, pk.cin_p, pk.cout, B, H, W), 64, 64, 3, (14, 736, 1280))),
    ("plan_wino", _other_shape("PackedWino", "conv2d_wino", lambda hb, pk, B, H, W: hb.wino_plan(pk.cin, pk.cout, B, H, W, False), 512, 512, 3,
                               (14, 92, 160))),
    ("plan_direct_ups", _other_tiles("PackedConv", "conv2d_ups", 64, 64, 3, ups=True)),
    ("plan_wino_ups", _other_tiles("PackedWino", "conv2d_ups_wino", 64, 64, 3, ups=True)),
    ("plan_wino1d", _other_tiles("PackedWino1d", "conv2d_wino1d", 32, 64, 5)),
    ("second_source_wino1d", _second_source("PackedWino1d", "conv2d_wino1d", 8, 32, 7)),
    ("second_source_wino5", _second_source("PackedWino5", "conv2d_wino5", 8, 32, 5)),
    ("second_source_wino7", _second_source("PackedWino7", "conv2d_wino7", 8, 32, 7)),
    ("ups_wino1d", lambda hb, dev: _pk(hb, dev, "PackedWino1d", 6, 32, 7, ups=True)),
    ("ups_wino5", lambda hb, dev: _pk(hb, dev, "PackedWino5", 8, 32, 5, ups=True)),
    ("ups_wino7", lambda hb, dev: _pk(hb, dev, "PackedWino7", 6, 32, 7, ups=True)),
    ("upgemm_not_ups", lambda hb, dev: _pk(hb, dev, "PackedUpGemm", 16, 32, 3, ups=False)),
    ("upgemm_unsupported_layer", lambda hb, dev: _pk(hb, dev, "PackedUpGemm", 16, 16, 3, ups=True)),
    ("kernel_size_wino", lambda hb, dev: _pk(hb, dev, "PackedWino", 16, 32, 5)),
    ("kernel_size_wino4", lambda hb, dev: _pk(hb, dev, "PackedWino4", 16, 32, 5)),
    ("kernel_size_wino1d", lambda hb, dev: _pk(hb, dev, "PackedWino1d", 16, 32, 3)),
    ("kernel_size_wino5", lambda hb, dev: _pk(hb, dev, "PackedWino5", 16, 32, 3)),
    ("kernel_size_wino7", lambda hb, dev: _pk(hb, dev, "PackedWino7", 16, 32, 5)),
    ("mask_with_activation", lambda hb, dev: hb._flags(True, True, object())),
]
REFUSAL_BY_ID = dict(REFUSALS)


def run_refusal(fn, dev):
    """-> "<exception type>: <message>" of the refusal (the test's own guards are AssertionErrors too: none of them may be what fired)."""
    from ssm_amd import hipbind as hb
    try:
        fn(hb, dev)
    except (AssertionError, RuntimeError) as e:
        msg = "%s: %s" % (type(e).__name__, e)
        assert "share a tile configuration" not in msg, msg
        return msg
    raise AssertionError("nothing was refused")


# ---- the whole model --------------------------------------------------------------------------------------------------------------------
def run_model(dev):
    """One stage-1 + stage-2 inference pass of the synthetic FullModel in mode f32w, 64x64, two interpolation times (the hoisted conv1a /
    conv7a parts and their pk_pair handles run) -> {"frames": digest, "layers": {"s<stage>[.pair].<layer>": [class, algo, bn, ck, cin_p,
    w.numel(), b.numel()]}}."""
    from models.superslomo_r import FullModel
    from ssm_amd.config import load_config, synthetic_weight_overrides
    from ssm_amd.weights import synthetic_frames, synthetic_state_dict
    ov = synthetic_weight_overrides()
    ov[("STAGE2", "CROSS_SKIP")] = "TRUE"
    m = FullModel(load_config("superslomo_original.ini", ov))
    m.stage1_model.load_state_dict(synthetic_state_dict(1, True))
    m.stage2_model.load_state_dict(synthetic_state_dict(2, True))
    m.precision = "f32w"
    m = m.to(dev).eval()
    frames = m.interpolate(synthetic_frames(2, 64, 64, seed=7).to(dev), [0.25, 0.75])
    torch.cuda.synchronize()
    eng = m._engine[1]
    layers = {}
    for plan in (eng.s1, eng.s2):
        for tag, pks in (("", plan.pk), (".pair", getattr(plan, "pk_pair", {}))):
            for name, pk in pks.items():
                layers["s%d%s.%s" % (plan.stage, tag, name)] = [type(pk).__name__, pk.algo, pk.bn, pk.ck, pk.cin_p, pk.w.numel(), pk.b.numel()]
    assert any(k.startswith("s2.pair.") for k in layers), "the stage-2 plan did not hoist its per-pair parts"
    return {"frames": digest(frames), "layers": layers}


# ---- the tests --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_covers_the_case_lists(recorded):
    assert len(recorded["commit"]) >= 7
    assert sorted(recorded["cases"]) == sorted(CASE_BY_ID) and sorted(recorded["refusals"]) == sorted(REFUSAL_BY_ID)


@pytest.mark.parametrize("cid", [c["id"] for c in CASES])
def test_form_is_bitwise_what_was_recorded(dev, recorded, cid):
    got = run_case(CASE_BY_ID[cid], dev)
    print(cid, got)
    assert got == recorded["cases"][cid]


@pytest.mark.parametrize("rid", [r[0] for r in REFUSALS])
def test_refusal_keeps_its_message(dev, recorded, rid):
    got = run_refusal(REFUSAL_BY_ID[rid], dev)
    print(rid, got)
    assert got == recorded["refusals"][rid]


def test_whole_model_is_bitwise_what_was_recorded(dev, recorded):
    got = run_model(dev)
    assert got["layers"] == recorded["model"]["layers"]
    assert got["frames"] == recorded["model"]["frames"]


def record(commit):
    dev = torch.device("cuda:0")
    out = {"commit": commit, "cases": {}, "refusals": {}}
    for c in CASES:
        a, b = run_case(c, dev), run_case(c, dev)
        if a != b:
            raise SystemExit("case %s is not repeatable: %s / %s - nothing written" % (c["id"], a, b))
        out["cases"][c["id"]] = a
        print(c["id"], a)
    for rid, fn in REFUSALS:
        out["refusals"][rid] = run_refusal(fn, dev)
        print(rid, out["refusals"][rid])
    a, b = run_model(dev), run_model(dev)
    if a != b:
        raise SystemExit("the model pass is not repeatable - nothing written")
    out["model"] = a
    path = os.environ.get("SSM_CONV_FORMS_DIGEST_OUT", FIXTURE)
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "superslomo-videointerpolation-pytorch_amd")
    for p in (root, pkg, os.path.join(pkg, "scripts")):
        if p not in sys.path:
            sys.path.insert(0, p)
    if "--record" not in sys.argv:
        raise SystemExit("usage: python tests/test_hip_conv_forms_digest.py --record [--commit ID]")
    record(sys.argv[sys.argv.index("--commit") + 1] if "--commit" in sys.argv else "unknown")
