"""The host-side argument checks of the fp32 convolution entry points (csrc/ssm_conv_host.h and the seven objects on top of it), held to
the return code and the FULL message of every refusal: one fully valid argument set per entry point at a one-tile problem, one thing broken
per case.  The pointers are made-up, suitably aligned integers - every case must be refused before anything is launched, and the module
skips itself where a GPU is present so that a regression can never turn a made-up pointer into a launch.  Also the forced-kind switches:
their counts, the clamp, and what the plan functions report under them."""
import ctypes
import types

import pytest
import torch

if torch.cuda.is_available():
    pytest.skip("made-up pointers: host-side refusals only, never on a machine that could launch", allow_module_level=True)

from ssm_amd import hipbind as hb  # noqa: E402

B, H, W = 2, 16, 32


def planes(ptr, C, h, w):
    hp, wp = hb.plane_dims(h, w)
    return hb.SsmView(ptr, C * hp * wp, hp * wp, wp)


def valid(cin=8, cout=32, ups=False, k=3, H=H, W=W):
    """The valid argument set: sources at the (half, for the fused-upsample forms) resolution, output / addend at H x W, pooled map at H/2 x W/2."""
    sh_, sw_ = (H // 2, W // 2) if ups else (H, W)
    return types.SimpleNamespace(
        x1=planes(0x10000000, cin, sh_, sw_), C1=cin, x2=hb.SsmView(None, 0, 0, 0), C2=0, w=0x20000000, bias=0x21000000,
        y=planes(0x30000000, cout, H, W), pool=planes(0x40000000, cout, H // 2, W // 2), add=planes(0x50000000, cout, H, W), add_div=1,
        B=B, H=H, W=W, Cout=cout, k=k, slope=0.1, flags=hb.SSM_FLAG_LRELU, ups=ups, srcW=sw_, cin=cin, KS=1, BN=32,
        scratch=hb.SsmView(0x60000000, 9 * cout * (H // 2) * (W // 2), (H // 2) * (W // 2), W // 2))


L = hb.load()
# entry -> (what its valid set differs in, call, has second source, has pool, has addend)
FORMS = {
    "conv_add": (dict(), lambda a: L.ssm_conv2d_add_fwd(a.x1, a.C1, a.x2, a.C2, a.w, a.bias, a.y, a.pool, a.add, a.add_div, a.B, a.H, a.W, a.Cout,
                                                         a.k, a.slope, a.flags, None), True, True, True),
    "conv_ups_add": (dict(ups=True), lambda a: L.ssm_conv2d_ups_add_fwd(a.x1, a.C1, a.x2, a.C2, a.w, a.bias, a.y, a.add, a.add_div, a.B, a.H, a.W,
                                                                         a.Cout, a.slope, a.flags, None), True, False, True),
    "wino_add": (dict(), lambda a: L.ssm_wino_conv2d_add_fwd(a.x1, a.C1, a.x2, a.C2, a.w, a.bias, a.y, a.pool, a.add, a.add_div, a.B, a.H, a.W,
                                                              a.Cout, a.slope, a.flags, None), True, True, True),
    "wino_ups_add": (dict(ups=True), lambda a: L.ssm_wino_conv2d_ups_add_fwd(a.x1, a.C1, a.x2, a.C2, a.w, a.bias, a.y, a.add, a.add_div, a.B, a.H,
                                                                              a.W, a.Cout, a.slope, a.flags, None), True, False, True),
    "wino_splitk": (dict(), lambda a: L.ssm_wino_conv2d_splitk_fwd(a.x1, a.C1, a.x2, a.C2, a.w, a.bias, a.y, a.KS, 0, a.B, a.H, a.W, a.Cout, a.BN,
                                                                    None), True, False, False),
    "wino4_add": (dict(), lambda a: L.ssm_wino4_conv2d_add_fwd(a.x1, a.C1, a.x2, a.C2, a.w, a.bias, a.y, a.pool, a.add, a.add_div, a.B, a.H, a.W,
                                                                a.Cout, a.slope, a.flags, None), True, True, True),
    "wino4_ups_add": (dict(ups=True), lambda a: L.ssm_wino4_conv2d_ups_add_fwd(a.x1, a.C1, a.x2, a.C2, a.w, a.bias, a.y, a.add, a.add_div, a.B,
                                                                                a.H, a.W, a.Cout, a.slope, a.flags, None), True, False, True),
    "wino4_ups_border": (dict(ups=True, H=32, W=64),          # (a border ring needs 2 x 2 workgroup tiles)
                         lambda a: L.ssm_wino4_conv2d_ups_border_fwd(a.x1, a.C1, a.x2, a.C2, a.w, a.bias, a.y, a.B, a.H, a.W,
                                                                                      a.Cout, a.slope, a.flags, None), True, False, False),
    "wino4_shuffle": (dict(cout=64), lambda a: L.ssm_wino4_conv2d_shuffle_fwd(a.x1, a.C1, a.x2, a.C2, a.w, a.bias, a.y, a.B, a.H, a.W, a.Cout,
                                                                               a.slope, a.flags, None), True, False, False),
    "wino1d_k5": (dict(k=5), lambda a: L.ssm_wino1d_conv2d_add_fwd(a.x1, a.C1, a.w, a.bias, a.y, a.pool, a.add, a.add_div, a.B, a.H, a.W, a.Cout,
                                                                    a.k, a.slope, a.flags, None), False, True, True),
    "wino1d_k7": (dict(k=7), lambda a: L.ssm_wino1d_conv2d_add_fwd(a.x1, a.C1, a.w, a.bias, a.y, a.pool, a.add, a.add_div, a.B, a.H, a.W, a.Cout,
                                                                    a.k, a.slope, a.flags, None), False, True, True),
    "wino5_add": (dict(), lambda a: L.ssm_wino5_conv2d_add_fwd(a.x1, a.C1, a.w, a.bias, a.y, a.pool, a.add, a.add_div, a.B, a.H, a.W, a.Cout,
                                                                a.slope, a.flags, None), False, True, True),
    "wino7_add": (dict(), lambda a: L.ssm_wino7_conv2d_add_fwd(a.x1, a.C1, a.w, a.bias, a.y, a.pool, a.add, a.add_div, a.B, a.H, a.W, a.Cout,
                                                                a.slope, a.flags, None), False, True, True),
    "upgemm_ups_add": (dict(ups=True), lambda a: L.ssm_upgemm_conv2d_ups_add_fwd(a.x1, a.C1, a.x2, a.C2, a.w, a.bias, a.scratch, a.y, a.add,
                                                                                  a.add_div, a.B, a.H, a.W, a.Cout, a.slope, a.flags, None),
                       True, False, True),
}


def second_source_other_sh(a):
    a.x2 = hb.SsmView(0x18000000, a.x1.sb, a.x1.sc, a.x1.sh + 4)
    a.C2 = a.C1


# mutation -> (breaks exactly one thing of the valid set, the forms it applies to: a predicate over (entry, two sources, pool, addend))
F22 = ("wino_add", "wino_ups_add", "wino_splitk")
UPS = ("conv_ups_add", "wino_ups_add", "wino4_ups_add", "wino4_ups_border", "upgemm_ups_add")
MUTATIONS = {
    "null x": (lambda a: setattr(a.x1, "ptr", None), lambda e, two, pool, add: True),
    "null y": (lambda a: setattr(a.y, "ptr", None), lambda e, two, pool, add: True),
    "null filter": (lambda a: setattr(a, "w", None), lambda e, two, pool, add: True),
    "x.ptr + 4": (lambda a: setattr(a.x1, "ptr", a.x1.ptr + 4), lambda e, two, pool, add: True),
    "x.sh + 2": (lambda a: setattr(a.x1, "sh", a.x1.sh + 2), lambda e, two, pool, add: True),
    "x.sh = W + 7": (lambda a: setattr(a.x1, "sh", a.srcW + 7), lambda e, two, pool, add: True),
    "x.sh = W + 4": (lambda a: setattr(a.x1, "sh", a.srcW + 4), lambda e, two, pool, add: True),          # (a multiple of 4: reaches the zero-frame check)
    "x.sc = 2^30": (lambda a: setattr(a.x1, "sc", 1 << 30), lambda e, two, pool, add: e != "wino7_add"),          # (wino7 bounds the ROW stride)
    "x.sh = 2^24": (lambda a: setattr(a.x1, "sh", 1 << 24), lambda e, two, pool, add: e == "wino7_add"),
    "x2.sh != x1.sh": (second_source_other_sh, lambda e, two, pool, add: two),
    "Cin + 1": (lambda a: setattr(a, "C1", a.C1 + 1), lambda e, two, pool, add: e not in ("upgemm_ups_add", "wino7_add")),          # (these take any channel count)
    "Cout = 33": (lambda a: setattr(a, "Cout", 33), lambda e, two, pool, add: e not in F22),          # (F(2x2) predicates its last cout block)
    "add_div = 3": (lambda a: setattr(a, "add_div", 3), lambda e, two, pool, add: add),
    "add_div = 0": (lambda a: setattr(a, "add_div", 0), lambda e, two, pool, add: add),
    "pool, H = 15": (lambda a: setattr(a, "H", 15), lambda e, two, pool, add: pool),
    "H = 15": (lambda a: setattr(a, "H", 15), lambda e, two, pool, add: e in UPS),
    "y.ptr + 4": (lambda a: setattr(a.y, "ptr", a.y.ptr + 4), lambda e, two, pool, add: e in F22),
    "add.ptr + 4": (lambda a: setattr(a.add, "ptr", a.add.ptr + 4), lambda e, two, pool, add: e in F22 and add),
    "B = 0": (lambda a: setattr(a, "B", 0), lambda e, two, pool, add: True),
}


def run_case(entry, mutation):
    base, call, _, _, _ = FORMS[entry]
    a = valid(**base)
    MUTATIONS[mutation][0](a)
    rc = call(a)
    return rc, L.ssm_last_error_string().decode()


def applicable():
    for entry, (_, _, two, pool, add) in FORMS.items():
        for mutation, (_, applies) in MUTATIONS.items():
            if applies(entry, two, pool, add):
                yield entry, mutation


# (entry, mutation, rc, message): recorded from the library before the entry points shared their prologue
ROWS = [
    ("conv_add", "null x", -1, 'conv: null pointer'),
    ("conv_add", "null y", -1, 'conv: null pointer'),
    ("conv_add", "null filter", -1, 'conv: null pointer'),
    ("conv_add", "x.ptr + 4", -1, 'conv: input 1 is not a padded-plane view (16-byte alignment)'),
    ("conv_add", "x.sh + 2", -1, 'conv: input 1 is not a padded-plane view (16-byte alignment)'),
    ("conv_add", "x.sh = W + 7", -1, 'conv: input 1 is not a padded-plane view (16-byte alignment)'),
    ("conv_add", "x.sh = W + 4", -1, 'conv: input 1 row stride 36 leaves no zero frame for W=32'),
    ("conv_add", "x.sc = 2^30", -1, 'conv: channel stride too large'),
    ("conv_add", "x2.sh != x1.sh", -1, 'conv: cat sources must share row/channel strides'),
    ("conv_add", "Cin + 1", -1, 'conv: channel counts (9,0) must be multiples of 8'),
    ("conv_add", "Cout = 33", -1, 'conv: the addend form needs Cout (33) to be a multiple of the cout block (32) of the tile configuration'),
    ("conv_add", "add_div = 3", -1, 'conv: the addend serves 3 batch entries each, batch 2 is no multiple'),
    ("conv_add", "add_div = 0", -1, 'conv: the addend serves 0 batch entries each, batch 2 is no multiple'),
    ("conv_add", "pool, H = 15", -1, 'conv: fused pool needs even H, W'),
    ("conv_add", "B = 0", -1, 'conv: bad batch'),
    ("conv_ups_add", "null x", -1, 'conv: null pointer'),
    ("conv_ups_add", "null y", -1, 'conv: null pointer'),
    ("conv_ups_add", "null filter", -1, 'conv: null pointer'),
    ("conv_ups_add", "x.ptr + 4", -1, 'conv: input 1 is not a padded-plane view (16-byte alignment)'),
    ("conv_ups_add", "x.sh + 2", -1, 'conv: input 1 is not a padded-plane view (16-byte alignment)'),
    ("conv_ups_add", "x.sh = W + 7", -1, 'conv: input 1 is not a padded-plane view (16-byte alignment)'),
    ("conv_ups_add", "x.sh = W + 4", -1, 'conv: input 1 row stride 20 leaves no zero frame for W=16'),
    ("conv_ups_add", "x.sc = 2^30", -1, 'conv: channel stride too large'),
    ("conv_ups_add", "x2.sh != x1.sh", -1, 'conv: cat sources must share row/channel strides'),
    ("conv_ups_add", "Cin + 1", -1, 'conv: channel counts (9,0) must be multiples of 8'),
    ("conv_ups_add", "Cout = 33", -1, 'conv: the addend form needs Cout (33) to be a multiple of the cout block (32) of the tile configuration'),
    ("conv_ups_add", "add_div = 3", -1, 'conv: the addend serves 3 batch entries each, batch 2 is no multiple'),
    ("conv_ups_add", "add_div = 0", -1, 'conv: the addend serves 0 batch entries each, batch 2 is no multiple'),
    ("conv_ups_add", "H = 15", -1, 'conv_ups: the output of a x2 upsample has even H, W (got 15x32)'),
    ("conv_ups_add", "B = 0", -1, 'conv_ups: bad batch'),
    ("wino_add", "null x", -1, 'wino conv: null pointer'),
    ("wino_add", "null y", -1, 'wino conv: null pointer'),
    ("wino_add", "null filter", -1, 'wino conv: null pointer'),
    ("wino_add", "x.ptr + 4", -1, 'wino conv: input 1 is not a padded-plane view (16-byte alignment)'),
    ("wino_add", "x.sh + 2", -1, 'wino conv: input 1 is not a padded-plane view (16-byte alignment)'),
    ("wino_add", "x.sh = W + 7", -1, 'wino conv: input 1 is not a padded-plane view (16-byte alignment)'),
    ("wino_add", "x.sh = W + 4", -1, 'wino conv: input 1 row stride 36 leaves no zero frame for W=32'),
    ("wino_add", "x.sc = 2^30", -1, 'wino conv: channel stride too large'),
    ("wino_add", "x2.sh != x1.sh", -1, 'wino conv: cat sources must share row/channel strides'),
    ("wino_add", "Cin + 1", -3, 'wino conv: no tile configuration for Cin=9 Cout=32 on a 16x32 map (needs Cin a multiple of 8)'),
    ("wino_add", "add_div = 3", -1, 'wino conv: the addend serves 3 batch entries each, batch 2 is no multiple'),
    ("wino_add", "add_div = 0", -1, 'wino conv: the addend serves 0 batch entries each, batch 2 is no multiple'),
    ("wino_add", "pool, H = 15", -1, 'wino conv: fused pool needs even H, W'),
    ("wino_add", "y.ptr + 4", -1, 'wino conv: output view must be 8-byte aligned (2x2 pixel blocks are stored as row pairs)'),
    ("wino_add", "add.ptr + 4", -1, 'wino conv: the addend view must be 8-byte aligned (read as row pairs)'),
    ("wino_add", "B = 0", -1, 'wino conv: bad batch'),
    ("wino_ups_add", "null x", -1, 'wino conv: null pointer'),
    ("wino_ups_add", "null y", -1, 'wino conv: null pointer'),
    ("wino_ups_add", "null filter", -1, 'wino conv: null pointer'),
    ("wino_ups_add", "x.ptr + 4", -1, 'wino conv: input 1 is not a padded-plane view (16-byte alignment)'),
    ("wino_ups_add", "x.sh + 2", -1, 'wino conv: input 1 is not a padded-plane view (16-byte alignment)'),
    ("wino_ups_add", "x.sh = W + 7", -1, 'wino conv: input 1 is not a padded-plane view (16-byte alignment)'),
    ("wino_ups_add", "x.sh = W + 4", -1, 'wino conv: input 1 row stride 20 leaves no zero frame for W=16'),
    ("wino_ups_add", "x.sc = 2^30", -1, 'wino conv: channel stride too large'),
    ("wino_ups_add", "x2.sh != x1.sh", -1, 'wino conv: cat sources must share row/channel strides'),
    ("wino_ups_add", "Cin + 1", -3, 'wino conv: no tile configuration for Cin=9 Cout=32 on a 16x32 map (needs Cin a multiple of 8)'),
    ("wino_ups_add", "add_div = 3", -1, 'wino conv: the addend serves 3 batch entries each, batch 2 is no multiple'),
    ("wino_ups_add", "add_div = 0", -1, 'wino conv: the addend serves 0 batch entries each, batch 2 is no multiple'),
    ("wino_ups_add", "H = 15", -1, 'wino conv_ups: the output of a x2 upsample has even H, W (got 15x32)'),
    ("wino_ups_add", "y.ptr + 4", -1, 'wino conv: output view must be 8-byte aligned (2x2 pixel blocks are stored as row pairs)'),
    ("wino_ups_add", "add.ptr + 4", -1, 'wino conv: the addend view must be 8-byte aligned (read as row pairs)'),
    ("wino_ups_add", "B = 0", -1, 'wino conv_ups: bad batch'),
    ("wino_splitk", "null x", -1, 'wino conv: null pointer'),
    ("wino_splitk", "null y", -1, 'wino conv: null pointer'),
    ("wino_splitk", "null filter", -1, 'wino conv: null pointer'),
    ("wino_splitk", "x.ptr + 4", -1, 'wino conv: input 1 is not a padded-plane view (16-byte alignment)'),
    ("wino_splitk", "x.sh + 2", -1, 'wino conv: input 1 is not a padded-plane view (16-byte alignment)'),
    ("wino_splitk", "x.sh = W + 7", -1, 'wino conv: input 1 is not a padded-plane view (16-byte alignment)'),
    ("wino_splitk", "x.sh = W + 4", -1, 'wino conv: input 1 row stride 36 leaves no zero frame for W=32'),
    ("wino_splitk", "x.sc = 2^30", -1, 'wino conv: channel stride too large'),
    ("wino_splitk", "x2.sh != x1.sh", -1, 'wino conv: cat sources must share row/channel strides'),
    ("wino_splitk", "Cin + 1", -3, 'wino conv_splitk: no two-workgroup configuration of 32 couts for Cin/KS = 9 on a 16x32 map'),
    ("wino_splitk", "y.ptr + 4", -1, 'wino conv: output view must be 8-byte aligned (2x2 pixel blocks are stored as row pairs)'),
    ("wino_splitk", "B = 0", -1, 'wino conv_splitk: bad batch / split (KS = 1, Cin = 8)'),
    ("wino4_add", "null x", -1, 'wino4 conv: null pointer'),
    ("wino4_add", "null y", -1, 'wino4 conv: null pointer'),
    ("wino4_add", "null filter", -1, 'wino4 conv: null pointer'),
    ("wino4_add", "x.ptr + 4", -1, 'wino4 conv: input 1 is not a padded-plane view (16-byte alignment)'),
    ("wino4_add", "x.sh + 2", -1, 'wino4 conv: input 1 is not a padded-plane view (16-byte alignment)'),
    ("wino4_add", "x.sh = W + 7", -1, 'wino4 conv: input 1 is not a padded-plane view (16-byte alignment)'),
    ("wino4_add", "x.sh = W + 4", -1, 'wino4 conv: input 1 row stride 36 leaves no zero frame for W=32'),
    ("wino4_add", "x.sc = 2^30", -1, 'wino4 conv: channel stride too large'),
    ("wino4_add", "x2.sh != x1.sh", -1, 'wino4 conv: cat sources must share row/channel strides'),
    ("wino4_add", "Cin + 1", -3, 'wino4 conv: no tile configuration for Cin=9 Cout=32 (Cin a multiple of 4, Cout a multiple of 32)'),
    ("wino4_add", "Cout = 33", -3, 'wino4 conv: no tile configuration for Cin=8 Cout=33 (Cin a multiple of 4, Cout a multiple of 32)'),
    ("wino4_add", "add_div = 3", -1, 'wino4 conv: the addend serves 3 batch entries each, batch 2 is no multiple'),
    ("wino4_add", "add_div = 0", -1, 'wino4 conv: the addend serves 0 batch entries each, batch 2 is no multiple'),
    ("wino4_add", "pool, H = 15", -1, 'wino4 conv: fused pool needs even H, W'),
    ("wino4_add", "B = 0", -1, 'wino4 conv: bad sizes'),
    ("wino4_ups_add", "null x", -1, 'wino4 conv: null pointer'),
    ("wino4_ups_add", "null y", -1, 'wino4 conv: null pointer'),
    ("wino4_ups_add", "null filter", -1, 'wino4 conv: null pointer'),
    ("wino4_ups_add", "x.ptr + 4", -1, 'wino4 conv: input 1 is not a padded-plane view (16-byte alignment)'),
    ("wino4_ups_add", "x.sh + 2", -1, 'wino4 conv: input 1 is not a padded-plane view (16-byte alignment)'),
    ("wino4_ups_add", "x.sh = W + 7", -1, 'wino4 conv: input 1 is not a padded-plane view (16-byte alignment)'),
    ("wino4_ups_add", "x.sh = W + 4", -1, 'wino4 conv: input 1 row stride 20 leaves no zero frame for W=16'),
    ("wino4_ups_add", "x.sc = 2^30", -1, 'wino4 conv: channel stride too large'),
    ("wino4_ups_add", "x2.sh != x1.sh", -1, 'wino4 conv: cat sources must share row/channel strides'),
    ("wino4_ups_add", "Cin + 1", -3, 'wino4 conv: no tile configuration for Cin=9 Cout=32 (Cin a multiple of 4, Cout a multiple of 32)'),
    ("wino4_ups_add", "Cout = 33", -3, 'wino4 conv: no tile configuration for Cin=8 Cout=33 (Cin a multiple of 4, Cout a multiple of 32)'),
    ("wino4_ups_add", "add_div = 3", -1, 'wino4 conv: the addend serves 3 batch entries each, batch 2 is no multiple'),
    ("wino4_ups_add", "add_div = 0", -1, 'wino4 conv: the addend serves 0 batch entries each, batch 2 is no multiple'),
    ("wino4_ups_add", "H = 15", -1, 'wino4 conv_ups: the output of a x2 upsample has even H, W (got 15x32)'),
    ("wino4_ups_add", "B = 0", -1, 'wino4 conv: bad sizes'),
    ("wino4_ups_border", "null x", -1, 'wino4 conv: null pointer'),
    ("wino4_ups_border", "null y", -1, 'wino4 conv: null pointer'),
    ("wino4_ups_border", "null filter", -1, 'wino4 conv: null pointer'),
    ("wino4_ups_border", "x.ptr + 4", -1, 'wino4 conv: input 1 is not a padded-plane view (16-byte alignment)'),
    ("wino4_ups_border", "x.sh + 2", -1, 'wino4 conv: input 1 is not a padded-plane view (16-byte alignment)'),
    ("wino4_ups_border", "x.sh = W + 7", -1, 'wino4 conv: input 1 is not a padded-plane view (16-byte alignment)'),
    ("wino4_ups_border", "x.sh = W + 4", -1, 'wino4 conv: input 1 row stride 36 leaves no zero frame for W=32'),
    ("wino4_ups_border", "x.sc = 2^30", -1, 'wino4 conv: channel stride too large'),
    ("wino4_ups_border", "x2.sh != x1.sh", -1, 'wino4 conv: cat sources must share row/channel strides'),
    ("wino4_ups_border", "Cin + 1", -1, 'wino4 conv_ups_border: Cin a multiple of 4, Cout of 32'),
    ("wino4_ups_border", "Cout = 33", -1, 'wino4 conv_ups_border: Cin a multiple of 4, Cout of 32'),
    ("wino4_ups_border", "H = 15", -1, 'wino4 conv_ups_border: the output of a x2 upsample has even H, W (got 15x64)'),
    ("wino4_ups_border", "B = 0", -1, 'wino4 conv: bad sizes'),
    ("wino4_shuffle", "null x", -1, 'wino4 conv: null pointer'),
    ("wino4_shuffle", "null y", -1, 'wino4 conv: null pointer'),
    ("wino4_shuffle", "null filter", -1, 'wino4 conv: null pointer'),
    ("wino4_shuffle", "x.ptr + 4", -1, 'wino4 conv: input 1 is not a padded-plane view (16-byte alignment)'),
    ("wino4_shuffle", "x.sh + 2", -1, 'wino4 conv: input 1 is not a padded-plane view (16-byte alignment)'),
    ("wino4_shuffle", "x.sh = W + 7", -1, 'wino4 conv: input 1 is not a padded-plane view (16-byte alignment)'),
    ("wino4_shuffle", "x.sh = W + 4", -1, 'wino4 conv: input 1 row stride 36 leaves no zero frame for W=32'),
    ("wino4_shuffle", "x.sc = 2^30", -1, 'wino4 conv: channel stride too large'),
    ("wino4_shuffle", "x2.sh != x1.sh", -1, 'wino4 conv: cat sources must share row/channel strides'),
    ("wino4_shuffle", "Cin + 1", -3, 'wino4 conv: no tile configuration for Cin=9 Cout=64 (Cin a multiple of 4, Cout a multiple of 32)'),
    ("wino4_shuffle", "Cout = 33", -1, 'wino4 conv_shuffle: 4 Cout (33) must be a multiple of 64'),
    ("wino4_shuffle", "B = 0", -1, 'wino4 conv: bad sizes'),
    ("wino1d_k5", "null x", -1, 'wino1d conv: null pointer'),
    ("wino1d_k5", "null y", -1, 'wino1d conv: null pointer'),
    ("wino1d_k5", "null filter", -1, 'wino1d conv: null pointer'),
    ("wino1d_k5", "x.ptr + 4", -1, 'wino1d conv: the input is not a padded-plane view (16-byte alignment)'),
    ("wino1d_k5", "x.sh + 2", -1, 'wino1d conv: the input is not a padded-plane view (16-byte alignment)'),
    ("wino1d_k5", "x.sh = W + 7", -1, 'wino1d conv: the input is not a padded-plane view (16-byte alignment)'),
    ("wino1d_k5", "x.sh = W + 4", -1, 'wino1d conv: input row stride 36 leaves no zero frame for W=32'),
    ("wino1d_k5", "x.sc = 2^30", -1, 'wino1d conv: channel stride too large'),
    ("wino1d_k5", "Cin + 1", -1, 'wino1d conv: the channel count (9) must be a multiple of 2 (pad the view)'),
    ("wino1d_k5", "Cout = 33", -3, 'wino1d conv: no tile configuration for k=5 Cin=8 Cout=33 (k = 7 / 5, Cout a multiple of 32)'),
    ("wino1d_k5", "add_div = 3", -1, 'wino1d conv: the addend serves 3 batch entries each, batch 2 is no multiple'),
    ("wino1d_k5", "add_div = 0", -1, 'wino1d conv: the addend serves 0 batch entries each, batch 2 is no multiple'),
    ("wino1d_k5", "pool, H = 15", -1, 'wino1d conv: fused pool needs even H, W'),
    ("wino1d_k5", "B = 0", -1, 'wino1d conv: bad sizes'),
    ("wino1d_k7", "null x", -1, 'wino1d conv: null pointer'),
    ("wino1d_k7", "null y", -1, 'wino1d conv: null pointer'),
    ("wino1d_k7", "null filter", -1, 'wino1d conv: null pointer'),
    ("wino1d_k7", "x.ptr + 4", -1, 'wino1d conv: the input is not a padded-plane view (16-byte alignment)'),
    ("wino1d_k7", "x.sh + 2", -1, 'wino1d conv: the input is not a padded-plane view (16-byte alignment)'),
    ("wino1d_k7", "x.sh = W + 7", -1, 'wino1d conv: the input is not a padded-plane view (16-byte alignment)'),
    ("wino1d_k7", "x.sh = W + 4", -1, 'wino1d conv: input row stride 36 leaves no zero frame for W=32'),
    ("wino1d_k7", "x.sc = 2^30", -1, 'wino1d conv: channel stride too large'),
    ("wino1d_k7", "Cin + 1", -1, 'wino1d conv: the channel count (9) must be a multiple of 2 (pad the view)'),
    ("wino1d_k7", "Cout = 33", -3, 'wino1d conv: no tile configuration for k=7 Cin=8 Cout=33 (k = 7 / 5, Cout a multiple of 32)'),
    ("wino1d_k7", "add_div = 3", -1, 'wino1d conv: the addend serves 3 batch entries each, batch 2 is no multiple'),
    ("wino1d_k7", "add_div = 0", -1, 'wino1d conv: the addend serves 0 batch entries each, batch 2 is no multiple'),
    ("wino1d_k7", "pool, H = 15", -1, 'wino1d conv: fused pool needs even H, W'),
    ("wino1d_k7", "B = 0", -1, 'wino1d conv: bad sizes'),
    ("wino5_add", "null x", -1, 'wino5 conv: null pointer'),
    ("wino5_add", "null y", -1, 'wino5 conv: null pointer'),
    ("wino5_add", "null filter", -1, 'wino5 conv: null pointer'),
    ("wino5_add", "x.ptr + 4", -1, 'wino5 conv: the input is not a padded-plane view (16-byte alignment)'),
    ("wino5_add", "x.sh + 2", -1, 'wino5 conv: the input is not a padded-plane view (16-byte alignment)'),
    ("wino5_add", "x.sh = W + 7", -1, 'wino5 conv: the input is not a padded-plane view (16-byte alignment)'),
    ("wino5_add", "x.sh = W + 4", -1, 'wino5 conv: input row stride 36 leaves no zero frame for W=32'),
    ("wino5_add", "x.sc = 2^30", -1, 'wino5 conv: channel stride too large'),
    ("wino5_add", "Cin + 1", -1, 'wino5 conv: the channel count (9) must be a multiple of 4 (pad the view)'),
    ("wino5_add", "Cout = 33", -3, 'wino5 conv: no tile configuration for Cin=8 Cout=33 (Cout a multiple of 32)'),
    ("wino5_add", "add_div = 3", -1, 'wino5 conv: the addend serves 3 batch entries each, batch 2 is no multiple'),
    ("wino5_add", "add_div = 0", -1, 'wino5 conv: the addend serves 0 batch entries each, batch 2 is no multiple'),
    ("wino5_add", "pool, H = 15", -1, 'wino5 conv: fused pool needs even H, W'),
    ("wino5_add", "B = 0", -1, 'wino5 conv: bad sizes'),
    ("wino7_add", "null x", -1, 'wino7 conv: null pointer'),
    ("wino7_add", "null y", -1, 'wino7 conv: null pointer'),
    ("wino7_add", "null filter", -1, 'wino7 conv: null pointer'),
    ("wino7_add", "x.ptr + 4", -1, 'wino7 conv: the input is not a padded-plane view (16-byte alignment)'),
    ("wino7_add", "x.sh + 2", -1, 'wino7 conv: the input is not a padded-plane view (16-byte alignment)'),
    ("wino7_add", "x.sh = W + 7", -1, 'wino7 conv: the input is not a padded-plane view (16-byte alignment)'),
    ("wino7_add", "x.sh = W + 4", -1, 'wino7 conv: input row stride 36 leaves no zero frame for W=32'),
    ("wino7_add", "x.sh = 2^24", -1, 'wino7 conv: row stride too large'),
    ("wino7_add", "Cout = 33", -3, 'wino7 conv: no tile configuration for Cin=8 Cout=33 (Cout a multiple of 32)'),
    ("wino7_add", "add_div = 3", -1, 'wino7 conv: the addend serves 3 batch entries each, batch 2 is no multiple'),
    ("wino7_add", "add_div = 0", -1, 'wino7 conv: the addend serves 0 batch entries each, batch 2 is no multiple'),
    ("wino7_add", "pool, H = 15", -1, 'wino7 conv: fused pool needs even H, W'),
    ("wino7_add", "B = 0", -1, 'wino7 conv: bad sizes'),
    ("upgemm_ups_add", "null x", -1, 'upgemm: null pointer'),
    ("upgemm_ups_add", "null y", -1, 'upgemm: null pointer'),
    ("upgemm_ups_add", "null filter", -1, 'upgemm: null pointer'),
    ("upgemm_ups_add", "x.ptr + 4", -1, 'upgemm: input 1 is not a padded-plane view (16-byte alignment)'),
    ("upgemm_ups_add", "x.sh + 2", -1, 'upgemm: input 1 is not a padded-plane view (16-byte alignment)'),
    ("upgemm_ups_add", "x.sh = W + 7", -1, 'upgemm: input 1 is not a padded-plane view (16-byte alignment)'),
    ("upgemm_ups_add", "x.sh = W + 4", -1, 'upgemm: input 1 row stride 20 leaves no frame for w=16'),
    ("upgemm_ups_add", "x.sc = 2^30", -1, 'upgemm: channel stride too large'),
    ("upgemm_ups_add", "x2.sh != x1.sh", -1, 'upgemm: cat sources must share row/channel strides'),
    ("upgemm_ups_add", "Cout = 33", -1, 'upgemm: unsupported problem (Cout = 33 must be a multiple of 32, H x W = 16 x 32 even)'),
    ("upgemm_ups_add", "add_div = 3", -1, 'upgemm: the addend serves 3 batch entries each, batch 2 is no multiple'),
    ("upgemm_ups_add", "add_div = 0", -1, 'upgemm: the addend serves 0 batch entries each, batch 2 is no multiple'),
    ("upgemm_ups_add", "H = 15", -1, 'upgemm: unsupported problem (Cout = 32 must be a multiple of 32, H x W = 15 x 32 even)'),
    ("upgemm_ups_add", "B = 0", -1, 'upgemm: bad batch / channel counts'),
]


def test_the_table_covers_every_applicable_case():
    assert sorted((e, m) for e, m, _, _ in ROWS) == sorted(applicable())


@pytest.mark.parametrize("entry,mutation,rc,message", ROWS, ids=["%s-%s" % (e, m.replace(" ", "")) for e, m, _, _ in ROWS])
def test_refusal(entry, mutation, rc, message):
    assert rc in (-1, -3), "a row of this table is a refusal on the host, never a launch"
    assert run_case(entry, mutation) == (rc, message)


def plan_kind(form, args):
    kind = ctypes.c_int(-7)
    tail = {"conv": 3, "wino": 3, "wino4": 3, "wino1d": 3, "wino5": 1, "wino7": 1}[form]
    outs = [ctypes.byref(kind)] + [None] * (tail - 1)
    assert getattr(L, "ssm_%s_plan" % form)(*args, *outs) == 0
    return kind.value


# form -> (number of kinds, arguments of its plan function for a problem on which kind 0 can be forced)
FORCE = {
    "conv": (15, (7, 8, 32, 2, 16, 32, 0, 0)),
    "wino": (12, (8, 32, 2, 16, 32, 0)),
    "wino4": (6, (64, 64, 7, 184, 320, 0)),
    "wino1d": (5, (7, 8, 32, 2, 16, 32)),
    "wino5": (2, (8, 32, 2, 16, 32)),
    "wino7": (4, (8, 32, 2, 16, 32)),
    "upgemm": (2, None),
}


@pytest.mark.parametrize("form", sorted(FORCE))
def test_forced_kind(form):
    n_kinds, args = FORCE[form]
    force = getattr(L, "ssm_%s_force_kind" % form)
    try:
        assert force(-1) == n_kinds
        if args is None:          # (no plan function: the GEMM's tile is chosen inside its entry point)
            assert force(n_kinds) == n_kinds and force(0) == n_kinds
            return
        unforced = plan_kind(form, args)
        assert force(n_kinds) == n_kinds, "out of range: clamped to automatic"
        assert plan_kind(form, args) == unforced
        assert force(-5) == n_kinds and plan_kind(form, args) == unforced
        assert force(0) == n_kinds
        assert plan_kind(form, args) == 0
    finally:
        force(-1)
