"""No-GPU checks of the low-res GEMM form of the decoder step conv3x3(upsample2x(cat[a, b])) (scripts/models/flow_computation.py:244-247;
csrc/ssm_upgemm.hip): the algebra it rests on, in torch fp32 against the oracle, and its place in the plan's algorithm choice."""
import pytest
import torch


def up_after_gemm(x, w, bias):
    """conv3x3(up(x)) as nine 1x1 convolutions of the LOW-res input, each upsampled (half-pixel rule, edge-clamped), shifted by its tap and
    zero outside the hi-res map - the form the kernels evaluate, in torch fp32."""
    import torch.nn.functional as F
    B, _, h, wd = x.shape
    H, W = 2 * h, 2 * wd
    out = bias.view(1, -1, 1, 1).expand(B, w.shape[0], H, W).clone()
    for u in range(3):
        for v in range(3):
            yuv = F.conv2d(x, w[:, :, u:u + 1, v:v + 1])
            up = F.interpolate(yuv, size=(H, W), mode="bilinear", align_corners=False)
            out += F.pad(up, (1, 1, 1, 1))[:, :, u:u + H, v:v + W]
    return out


@pytest.mark.parametrize("h,w,cin,cout", [(3, 5, 64, 32), (7, 9, 64, 32), (12, 20, 1024, 32), (23, 40, 512, 32)])
def test_upsample_and_tap_matrices_commute(h, w, cin, cout):
    from oracle import ssm_oracle as O
    g = torch.Generator().manual_seed(h * w)
    x = torch.randn(2, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5
    bias = torch.randn(cout, generator=g) * 0.1
    pre = up_after_gemm(x, wt, bias)
    got = torch.where(pre >= 0, pre, pre * O.LRELU_SLOPE)
    want = O.conv2d_lrelu(O.upsample2x_bilinear(x), wt, bias)
    e = float((got - want).abs().max())
    assert e < 5e-6, e


def test_choose_algo_selects_the_form_only_for_fused_upsample_layers_of_inference_plans():
    from ssm_amd import engine as E
    old = E.UPGEMM
    try:
        E.UPGEMM = "conv8a,conv3a"
        args = (1024, 256, 3, 14, 92, 160)
        assert E.choose_algo("conv8a", *args, True, True, True) == "upgemm"
        assert E.choose_algo("conv8a", *args, False, True, True) != "upgemm"          # not a fused-upsample launch
        assert E.choose_algo("conv3a", 64, 128, 3, 14, 184, 320, False, True, True) != "upgemm"
        assert E.choose_algo("conv8a", *args, True, True, False) != "upgemm"          # training plan (no 1-D / inference-only forms)
        assert E.choose_algo("conv8a", *args, True, False, False) == "direct"         # mode f32
        assert E.choose_algo("conv9a", 512, 128, 3, 14, 184, 320, True, True, True) != "upgemm"      # not in the list
        assert E.choose_algo("conv8a", *args, True, True, True, upgemm=False) != "upgemm"
        E.UPGEMM = "0"
        assert E.choose_algo("conv8a", *args, True, True, True) != "upgemm"
        E.UPGEMM = "1"          # by the library's rule: a pure function of the problem
        assert E.choose_algo("conv8a", *args, True, True, True) == E.choose_algo("conv8a", *args, True, True, True)
        assert E.choose_algo("conv11a", 128, 32, 3, 14, 736, 1280, True, True, True) != "upgemm"      # the 9 Cout intermediate does not pay
    finally:
        E.UPGEMM = old


def test_issued_factor_and_launcher():
    from ssm_amd import engine as E
    from ssm_amd import hipbind as hb
    assert E.ISSUED_FACTOR["upgemm"](3) == 0.25
    assert E._ALGO_CLASS["upgemm"]() is hb.PackedUpGemm

    class Pk:
        algo = "upgemm"
    assert E.conv_fn(Pk, True) is hb.conv2d_ups_upgemm
