"""No-GPU checks of the table of fp32 convolution forms (ssm_amd/hipbind.py): every layer of both U-Nets still gets the form recorded in
tests/golden/conv_forms_choice.json (engine.choose_algo is host code: the library's plan and cost functions need no device), and the tables
derived from the forms hold the values they held when they were written out by hand.

    python tests/test_conv_forms_table_cpu.py --record [--commit ID]

writes the fixture; it uses only names the recorded commit has as well."""
import json
import os
import sys

import pytest

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_forms_choice.json")

SIZES = ((736, 1280, 14), (736, 1280, 7), (352, 352, 2))
# (wino1d, wino4, blocked2d) of a mode-f32w plan (engine.UNetPlan.__init__)
SETTINGS = {"inference": (True, True, True), "training": (False, True, True)}


def chosen_forms():
    """{"<setting> s<stage> <H>x<W> b<B>": {layer: form}} for every layer of both U-Nets (decoder and encoder at the same batch)."""
    from ssm_amd import engine as E
    from ssm_amd.weights import unet_layers
    out = {}
    for setting, (wino1d, wino4, blocked2d) in SETTINGS.items():
        for stage in (1, 2):
            for H, W, B in SIZES:
                forms = {}
                for name, ci, co, k in unet_layers(stage, True):
                    s = E.layer_scale(name)
                    forms[name] = E.choose_algo(name, ci, co, k, B, H // s, W // s, name in E.UNetPlan.UPS, True, wino1d, wino4, blocked2d)
                out["%s s%d %dx%d b%d" % (setting, stage, H, W, B)] = forms
    return out


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_every_layer_gets_the_recorded_form(recorded):
    got = chosen_forms()
    assert sorted(got) == sorted(recorded["forms"])
    for key, forms in got.items():
        assert forms == recorded["forms"][key], key
    used = {a for forms in got.values() for a in forms.values()}
    assert used >= {"direct", "wino", "wino4", "wino5", "wino7", "upgemm"}, used


FORMS = ("direct", "wino", "wino4", "wino1d", "wino5", "wino7", "upgemm")


def test_issued_factor_per_form_and_kernel_size():
    from ssm_amd import engine as E
    want = {"direct": lambda k: 1.0, "wino": lambda k: 16.0 / 36.0, "wino4": lambda k: 36.0 / 144.0,
            "wino1d": lambda k: 8.0 / 14.0 if k == 7 else 8.0 / 20.0, "wino7": lambda k: 196.0 / 784.0,
            "wino5": lambda k: 64.0 / 400.0, "upgemm": lambda k: 9.0 / 36.0}
    assert sorted(E.ISSUED_FACTOR) == sorted(FORMS)
    for a in FORMS:
        for k in (3, 5, 7):
            assert E.ISSUED_FACTOR[a](k) == want[a](k), (a, k)

    class Pk:
        algo, k = "wino1d", 7
    assert E.issued_factor(Pk) == 8.0 / 14.0

    class Pk16:          # (a handle without a form: the fp16 / Q8 filters)
        k = 3
    assert E.issued_factor(Pk16) == 1.0


def test_every_form_name_maps_to_the_class_of_that_name():
    from ssm_amd import engine as E
    from ssm_amd import hipbind as hb
    names = {"direct": "PackedConv", "wino": "PackedWino", "wino4": "PackedWino4", "wino1d": "PackedWino1d", "wino5": "PackedWino5",
             "wino7": "PackedWino7", "upgemm": "PackedUpGemm"}
    assert sorted(E._ALGO_CLASS) == sorted(names)
    for a, n in names.items():
        cls = E._ALGO_CLASS[a]()
        assert cls is getattr(hb, n) and cls.__name__ == n and cls.algo == a
    assert hb.PackedSubpixelWino4.algo == "wino4"


def test_launcher_of_every_form():
    from ssm_amd import engine as E
    from ssm_amd import hipbind as hb
    plain = {"direct": hb.conv2d, "wino": hb.conv2d_wino, "wino4": hb.conv2d_wino4, "wino1d": hb.conv2d_wino1d, "wino5": hb.conv2d_wino5,
             "wino7": hb.conv2d_wino7}
    ups = {"direct": hb.conv2d_ups, "wino": hb.conv2d_ups_wino, "wino4": hb.conv2d_ups_wino4, "upgemm": hb.conv2d_ups_upgemm}
    for a in FORMS:
        Pk = type("Pk", (), {"algo": a})
        if a in plain:
            assert E.conv_fn(Pk) is plain[a], a
        if a in ups:
            assert E.conv_fn(Pk, True) is ups[a], a
    with pytest.raises(AssertionError, match="the low-res GEMM form is for the fused-upsample layers"):
        E.conv_fn(type("Pk", (), {"algo": "upgemm"}))


def test_batch_repack_job_ids_and_tiled_forms():
    from ssm_amd import hipbind as hb
    assert hb.PackBatch32.ALGO == {"direct": 0, "wino": 1, "wino1d": 2, "wino4": 3, "wino7": 4, "wino5": 5}

    def pk(algo, bn, cout=64, cin=32, per=None, **kw):
        w = type("W", (), {"numel": staticmethod(lambda: (cout // (32 if algo == "wino4" else bn)) * cin * per * (32 if algo == "wino4" else bn))})
        return type("Pk", (), dict(algo=algo, bn=bn, k=3, cout=cout, cin=cin, cin_p=cin, w=w, **kw))
    # packed floats per (cout, cin) of the three forms the tiled repack kernel knows; F(4x4,3x3) always in 32-cout blocks
    assert hb.PackBatch32._tiled(pk("direct", 32, per=9)) and hb.PackBatch32._tiled(pk("wino", 64, per=16))
    assert hb.PackBatch32._tiled(pk("wino4", 128, per=36)) and hb.PackBatch32._tile_bn(pk("wino4", 128, per=36)) == 32
    assert hb.PackBatch32._tile_bn(pk("wino", 64, per=16)) == 64
    assert not hb.PackBatch32._tiled(pk("wino", 64, per=9)) and not hb.PackBatch32._tiled(pk("wino5", 32, per=16))
    assert not hb.PackBatch32._tiled(pk("direct", 32, cin=24, per=9)) and not hb.PackBatch32._tiled(pk("direct", 16, per=9))


def record(commit):
    with open(FIXTURE, "w") as f:
        json.dump({"commit": commit, "forms": chosen_forms()}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", FIXTURE)


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "superslomo-videointerpolation-pytorch_amd")
    for p in (root, pkg, os.path.join(pkg, "scripts")):
        if p not in sys.path:
            sys.path.insert(0, p)
    if "--record" not in sys.argv:
        raise SystemExit("usage: python tests/test_conv_forms_table_cpu.py --record [--commit ID]")
    record(sys.argv[sys.argv.index("--commit") + 1] if "--commit" in sys.argv else "unknown")
