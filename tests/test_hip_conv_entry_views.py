"""The `vec` decision of the convolution entry points that compute it (F(4x4,3x3), F(4x4,5x5), the blocked 7x7 form, the 1-D form for 5x5 and
7x7; csrc/ssm_conv_host.h): may the epilogue move the outputs, the addend and the pooled outputs as aligned 16- / 8-byte pieces?  Each form
runs once into aligned views and once with ONE of the three views shifted by a pixel, so that the element-wise epilogue must be chosen.  The
arithmetic is the same and only the store width differs: the results are compared BITWISE on the H x W window, and everything outside the
window must still be zero.  No tolerance is involved."""
import pytest
import torch

from ssm_amd import hipbind as hb

pytestmark = pytest.mark.gpu

B, H, W, COUT = 2, 16, 36, 32          # one 16 x 32-pixel workgroup tile plus a ragged one

# form -> (filter size, Cin: the smallest the form takes, packed-filter class, launch)
FORMS = {
    "wino4": (3, 8, hb.PackedWino4, hb.conv2d_wino4),
    "wino5": (5, 1, hb.PackedWino5, hb.conv2d_wino5),
    "wino7": (7, 1, hb.PackedWino7, hb.conv2d_wino7),
    "wino1d_k5": (5, 1, hb.PackedWino1d, hb.conv2d_wino1d),
    "wino1d_k7": (7, 1, hb.PackedWino1d, hb.conv2d_wino1d),
}


def window(p, h, w, x0):
    return p.full[:, :, hb.SSM_PADY:hb.SSM_PADY + h, hb.SSM_PADX + x0:hb.SSM_PADX + x0 + w]


def only_window_written(p, h, w, x0):
    rest = p.buf.clone()
    rest[:p.full.numel()].view_as(p.full)[:, :, hb.SSM_PADY:hb.SSM_PADY + h, hb.SSM_PADX + x0:hb.SSM_PADX + x0 + w] = 0
    return not bool(rest.any())          # (frame, the columns beside the window and the tail slack)


@pytest.mark.parametrize("form", sorted(FORMS))
def test_shifted_views_take_the_elementwise_epilogue_bitwise(form):
    k, cin, Packed, launch = FORMS[form]
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(11)
    wt = (torch.randn(COUT, cin, k, k, generator=g) / (k * cin ** 0.5)).to(dev)
    bs = torch.randn(COUT, generator=g).to(dev)
    pk = Packed(wt, bs, B, H, W, pool=True)
    cin_p = getattr(pk, "cin_p", cin)          # (channels beyond Cin: zero planes the packed filter ignores)
    x = torch.zeros(B, cin_p, H, W)
    x[:, :cin] = torch.randn(B, cin, H, W, generator=g)
    xin = hb.Planes(B, cin_p, H, W, dev).load(x.to(dev))          # the input view stays aligned
    addend = torch.randn(B, COUT, H, W, generator=g).to(dev)

    def run(ys, as_, ps):
        """One launch with the output / addend / pooled view shifted by ys / as_ / ps pixels; -> (output planes, pooled planes)."""
        y = hb.Planes(B, COUT, H, W + 4, dev)
        a = hb.Planes(B, COUT, H, W + 4, dev)
        q = hb.Planes(B, COUT, H // 2, W // 2 + 4, dev)
        window(a, H, W, as_).copy_(addend)
        launch(xin.view(), cin_p, None, 0, pk, y.view(x0=ys), q.view(x0=ps), B, H, W, add=a.view(x0=as_))
        torch.cuda.synchronize()
        assert only_window_written(y, H, W, ys) and only_window_written(q, H // 2, W // 2, ps)
        return window(y, H, W, ys).contiguous().view(torch.int32), window(q, H // 2, W // 2, ps).contiguous().view(torch.int32)

    want_y, want_q = run(0, 0, 0)
    assert bool(want_y.any()) and bool(want_q.any())
    for shift in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
        got_y, got_q = run(*shift)
        assert torch.equal(got_y, want_y), "output differs with (y, add, pool) shifted by %r" % (shift,)
        assert torch.equal(got_q, want_q), "pooled output differs with (y, add, pool) shifted by %r" % (shift,)
