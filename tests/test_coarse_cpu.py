"""No-GPU checks of the coarse-flow mode (flow_scale = 2 | 4): the entry point is declared, exported and bound; the source
indices and weights of the map upsampling (ssm_amd.coarse.upscale_taps: the rule the kernel evaluates per lane) as literal values and
against torch.nn.functional.interpolate in float64; the canvas sizes; the refusals; the float64 reference of the GPU tests against its
own float32 evaluation."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "ssm_synthesize_upscaled_fwd"


def test_entry_point_is_declared_exported_and_bound():
    from ssm_amd import hipbind as hb
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ssm_hip.h")).read(), flags=re.S)
    m = re.search(r"int\s+%s\s*\(([^)]*)\)" % ENTRY, src)
    assert m, "include/ssm_hip.h does not declare %s" % ENTRY
    args = [a.strip() for a in m.group(1).split(",")]
    assert args == ["ssm_view img6", "ssm_view aux_lo", "const float *t", "ssm_view y3", "int B", "int H", "int W", "int s", "void *stream"]
    out = subprocess.run(["nm", "-D", "--defined-only", hb.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert any(ln.split()[-1] == ENTRY and " T " in ln for ln in out.splitlines()), "libssm_hip.so does not export %s" % ENTRY
    res, argtypes = hb.SIGNATURES[ENTRY]
    assert len(argtypes) == len(args) and argtypes[:2] == [hb.SsmView, hb.SsmView] and argtypes[3] == hb.SsmView
    assert hasattr(hb.load(), ENTRY)


def test_entry_point_refuses_bad_arguments_by_name():
    """Host-side argument checks: no launch, no GPU needed.  The pointers are made up, so where a GPU is present the test skips itself (a
    regression must never turn one into a launch); tests/test_hip_coarse.py asks the same refusals with real tensors there."""
    if torch.cuda.is_available():
        pytest.skip("made-up pointers: host-side refusals only, never on a machine that could launch")
    from ssm_amd import hipbind as hb
    lib = hb.load()
    null = hb.SsmView(None, 0, 0, 0)
    some = hb.SsmView(4096, 6 * 64, 64, 8)          # never dereferenced: every call below is refused before the launch
    fn = getattr(lib, ENTRY)
    err = lambda: lib.ssm_last_error_string().decode()  # noqa: E731
    assert fn(some, some, 4096, some, 1, 8, 8, 3, None) == -1 and "s must be 2 or 4" in err()
    assert fn(some, some, 4096, some, 1, 8, 8, 1, None) == -1 and "s must be 2 or 4" in err()
    assert fn(some, some, 4096, some, 1, 8, 10, 4, None) == -1 and "multiples of s" in err()
    assert fn(some, some, 4096, some, 1, 7, 8, 2, None) == -1 and "multiples of s" in err()
    assert fn(null, some, 4096, some, 1, 8, 8, 2, None) == -1 and "img6" in err()
    assert fn(some, null, 4096, some, 1, 8, 8, 2, None) == -1 and "aux_lo" in err()
    assert fn(some, some, None, some, 1, 8, 8, 2, None) == -1 and "t is a null" in err()
    assert fn(some, some, 4096, null, 1, 8, 8, 2, None) == -1 and "y3" in err()
    assert fn(some, some, 4096, some, 0, 8, 8, 2, None) == -1 and "bad sizes" in err()


def test_upscale_taps_literal_values():
    from ssm_amd.coarse import upscale_taps
    i0, i1, lam = upscale_taps(3, 2)          # rows 0..5 of a 3-row map at s = 2
    assert i0.tolist() == [0, 0, 0, 1, 1, 2]
    assert i1.tolist() == [1, 1, 1, 2, 2, 2]          # row 5: clamped at h - 1
    assert lam.tolist() == [0.0, 0.25, 0.75, 0.25, 0.75, 0.25]
    # row 0: the position is clamped (max(0, -0.25) = 0), not the index: i1 = min(0 + 1, h - 1) = 1 carries weight 0, so the row is
    # source row 0 alone
    assert (i0[0], i1[0], lam[0]) == (0, 1, 0.0) and (i0[5], i1[5]) == (2, 2)
    i0, i1, lam = upscale_taps(2, 4)          # 8 outputs of a 2-sample axis at s = 4
    assert i0.tolist() == [0, 0, 0, 0, 0, 0, 1, 1]
    assert i1.tolist() == [1, 1, 1, 1, 1, 1, 1, 1]
    assert lam.tolist() == [0.0, 0.0, 0.125, 0.375, 0.625, 0.875, 0.125, 0.375]
    for s, allowed in ((2, {0.0, 0.25, 0.75}), (4, {0.0, 0.125, 0.375, 0.625, 0.875})):
        _, _, lam = upscale_taps(9, s)
        assert set(lam.tolist()) == allowed and lam.dtype == np.float32
        assert set(lam[s:-s].tolist()) == allowed - {0.0}          # away from the top edge no weight is zero
    i0, i1, lam = upscale_taps(1, 4)          # one source sample: both taps are that sample
    assert i0.tolist() == [0] * 4 and i1.tolist() == [0] * 4


@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 33])
def test_upscale_taps_are_torch_interpolate_in_float64(s, n):
    """A ramp makes every index and weight visible; a random signal holds the composition.  Exact: the weights are multiples of 1/8."""
    from ssm_amd.coarse import upscale_taps
    i0, i1, lam = upscale_taps(n, s)
    lam = lam.astype(np.float64)
    for sig in (np.arange(n, dtype=np.float64) * 3.0 + 1.0, np.random.RandomState(n).rand(n)):
        want = torch.nn.functional.interpolate(torch.from_numpy(sig).view(1, 1, 1, n), scale_factor=(1, s), mode="bilinear",
                                               align_corners=False).view(-1).numpy()
        got = (1.0 - lam) * sig[i0] + lam * sig[i1]
        assert np.abs(got - want).max() <= 1e-15 * np.abs(sig).max()


@pytest.mark.parametrize("s", [2, 4])
def test_host_yardstick_of_the_map_sampling(s):
    """upsample_maps_host (float32, columns first and then rows) within float32 rounding of F.interpolate in float64 on a 2-D signal."""
    from ssm_amd.coarse import upsample_maps_host
    m = np.random.RandomState(3).randn(2, 5, 5, 7).astype(np.float32)
    want = torch.nn.functional.interpolate(torch.from_numpy(m).double(), scale_factor=s, mode="bilinear", align_corners=False).numpy()
    got = upsample_maps_host(m, s)
    assert got.dtype == np.float32 and got.shape == (2, 5, 5 * s, 7 * s)
    assert np.abs(got - want).max() <= 4 * 2.0 ** -24 * np.abs(m).max()


def test_canvas_sizes():
    from ssm_amd.frames import padded_dims
    from ssm_amd.video import VideoInterpolator
    assert padded_dims(720, 1280, 64) == ((768, 1280), (24, 0))
    assert padded_dims(720, 1280, 128) == ((768, 1280), (24, 0))
    assert padded_dims(2160, 3840, 64) == ((2176, 3840), (8, 0))
    assert padded_dims(2160, 3840, 128) == ((2176, 3840), (8, 0))
    assert padded_dims(720, 1280) == ((736, 1280), (8, 0)) and padded_dims(96, 160, 64) == ((128, 192), (16, 16))
    from ssm_amd.config import load_config, synthetic_weight_overrides
    cfg = load_config("superslomo_original.ini", synthetic_weight_overrides())
    for s in (1, 2, 4):
        vi = VideoInterpolator(None, cfg, flow_scale=s)
        for h, w in ((720, 1280), (2160, 3840), (96, 160)):
            assert vi.canvas(h, w) == padded_dims(h, w, 32 * s)[0]
    assert VideoInterpolator(None, cfg).canvas(96, 160) == (96, 160)


def test_refusals():
    from models.superslomo_r import FullModel
    from ssm_amd.coarse import check_scale, size_rule
    from ssm_amd.config import load_config, synthetic_weight_overrides
    from ssm_amd.engine import CoarseFlowEngine, PairPipeline
    from ssm_amd.video import VideoInterpolator
    for bad in (0, 3, 8, -2, 2.5, "2", None):
        with pytest.raises(ValueError, match="flow_scale must be 1, 2 or 4"):
            check_scale(bad)
    assert [check_scale(s) for s in (1, 2, 4)] == [1, 2, 4]
    assert size_rule(128, 256, 4) == (32, 64) and size_rule(128, 192, 2) == (64, 96)
    for H, W, s in ((96, 128, 2), (128, 160, 2), (128, 192, 4), (736, 1280, 2)):
        with pytest.raises(AssertionError, match=r"multiples of 32\*flow_scale = %d" % (32 * s)):
            size_rule(H, W, s)
    dev = torch.device("cpu")          # every refusal below comes before anything is allocated
    with pytest.raises(AssertionError, match=r"multiples of 32\*flow_scale = 64"):
        CoarseFlowEngine({}, {}, 1, 3, 96, 128, dev, 2)
    with pytest.raises(ValueError, match="flow_scale must be 1, 2 or 4"):
        CoarseFlowEngine({}, {}, 1, 3, 128, 128, dev, 3)
    with pytest.raises(AssertionError, match="flow_scale=1 is the plain PairEngine"):
        CoarseFlowEngine({}, {}, 1, 3, 128, 128, dev, 1)
    with pytest.raises(ValueError, match="flow_scale must be 1, 2 or 4"):
        PairPipeline({}, {}, 3, 128, 128, dev, flow_scale=3)
    with pytest.raises(NotImplementedError, match=r"graphs=True\) does not cover flow_scale=2"):
        PairPipeline({}, {}, 3, 128, 128, dev, graphs=True, flow_scale=2)
    cfg = load_config("superslomo_original.ini", synthetic_weight_overrides())
    with pytest.raises(ValueError, match="flow_scale must be 1, 2 or 4"):
        VideoInterpolator(None, cfg, flow_scale=3)
    fm = FullModel(cfg)
    with pytest.raises(ValueError, match="flow_scale must be 1, 2 or 4"):
        fm._flow_scale(3)
    assert fm._flow_scale(2) == 2
    rec = FullModel(load_config("superslomo_recurrent.ini", synthetic_weight_overrides()))
    assert rec._flow_scale(1) == 1
    with pytest.raises(NotImplementedError, match="flow_scale=2 is not available with a recurrent bottleneck"):
        rec._flow_scale(2)
    with pytest.raises(NotImplementedError, match="recurrent bottleneck"):
        VideoInterpolator(rec, cfg, flow_scale=4)


def test_cli_flags():
    import interpolate_video
    import visualize_interpolation
    base = ["-c", "x.ini", "--expt", "e", "--log", "l"]
    a = interpolate_video.getargs(base + ["--input", "-", "--output", "-"])
    assert a.flow_scale == 1
    assert interpolate_video.getargs(base + ["--input", "-", "--output", "-", "--flow_scale", "4"]).flow_scale == 4
    vis = base + ["--input_dir", "i", "--img_type", "png", "--output_dir", "o"]
    assert visualize_interpolation.getargs(vis).flow_scale == 1 and visualize_interpolation.getargs(vis + ["--flow_scale", "2"]).flow_scale == 2
    with pytest.raises(SystemExit):
        interpolate_video.getargs(base + ["--input", "-", "--output", "-", "--flow_scale", "3"])


def test_reference_is_a_usable_yardstick():
    """tests/coarse_refs.py: the float32 evaluation of the reference sits at float32 rounding from the float64 one on both families (so
    the 4 d bar of the GPU tests is a tight one), the outside family does leave the frame on every side and both keep the denominator
    away from zero."""
    import coarse_refs as R
    for h, w, s in ((3, 5, 2), (5, 33, 4), (7, 40, 2)):
        for fam in R.FAMILIES:
            c = R.kernel_case(h, w, s, fam)
            for form in ("each", "bcast"):
                want, d, bound = c[form]
                assert tuple(want.shape) == (3, 3, s * h, s * w) and want.dtype == torch.float64 and bool(torch.isfinite(want).all())
                assert 0.0 < d < 1e-3 and bound == max(4 * d, 1e-6), (h, w, s, fam, d)
            assert 0.05 <= float(c["aux"][:, 4].min()) and float(c["aux"][:, 4].max()) <= 0.95
            if fam == "outside":
                up = s * torch.nn.functional.interpolate(c["aux"][:, 0:4], scale_factor=s, mode="bilinear", align_corners=False)
                xs = torch.arange(c["W"]).view(1, 1, -1) + up[:, 2]
                ys = torch.arange(c["H"]).view(1, -1, 1) + up[:, 3]
                assert xs.min() < -1 and xs.max() > c["W"] and ys.min() < -1 and ys.max() > c["H"]
