"""Host-side references and case tables for the fp16 / fp8 convolution family (csrc/ssm_conv16.hip), shared by
tests/test_hip_conv16_kinds.py, tests/test_hip_hl8_layout.py (GPU) and tests/test_conv16_kinds_cpu.py (no GPU).

A plain helper module (no fixtures, no collection hooks).  Three parts:

1. The HL8 and Q8 encodings written from the comments in include/ssm_hip.h, on raw buffers:
     HL8  [B][G][hi|lo][Hp][Wp][8 x fp16]                        x = hi + lo,  hi = fp16(x), lo = fp16(x - hi)
     Q8   the same hi planes; plane 1 of the EVEN group of a pair holds [8 x e4m3(x) even | 8 x e4m3(x) odd], plane 1 of the ODD
          group [8 x e4m3((x - hi) * 2^11) even | odd]            x ~= hi + e4m3(..) * 2^-11, both e4m3 values clamped to +-448
   The e4m3 (OCP "fn": bias 7, no infinities, 448 largest) rounding is an explicit table: round to nearest, ties to the even code.
2. The case table of the convolution tests: per tile kind the smallest shapes that reach each decision of the kernel.
3. Exact-integer inputs and their int64 / float64 convolution.
"""
import torch
import torch.nn.functional as F

PADY, PADX = 3, 4           # SSM_PADY, SSM_PADX (include/ssm_hip.h); asserted against hipbind by the GPU modules
F64 = torch.float64


# ---- 1. encodings ------------------------------------------------------------------------------------------------------------------
def _e4m3_table():
    t = torch.zeros(256, dtype=F64)
    for code in range(256):
        s, e, m = code >> 7, (code >> 3) & 15, code & 7
        if e == 15 and m == 7:
            v = float("nan")
        elif e == 0:
            v = m / 8.0 * 2.0 ** -6
        else:
            v = (1 + m / 8.0) * 2.0 ** (e - 7)
        t[code] = -v if s else v
    return t


E4M3 = _e4m3_table()
_POS = E4M3[:127].clone()                   # codes 0..126: 0 .. 448, increasing


def e4m3_decode(codes):
    """uint8 codes -> float64."""
    return E4M3[codes.long()]


def e4m3_encode(x):
    """float tensor -> uint8 codes: clamp to +-448, round to nearest, ties to the even code; the sign bit follows the input's."""
    x = x.to(F64)
    neg = torch.signbit(x)
    a = x.abs().clamp(max=448.0)
    hi = torch.searchsorted(_POS, a).clamp(max=126)          # first code with value >= a
    lo = (hi - 1).clamp(min=0)
    dlo, dhi = a - _POS[lo], _POS[hi] - a
    pick_hi = (dhi < dlo) | ((dhi == dlo) & (hi % 2 == 0))
    code = torch.where(pick_hi, hi, lo)
    return (code + neg.long() * 128).to(torch.uint8)


def split_hl(x):
    """(hi, lo) fp16 tensors of an fp32 tensor, by the header's rule, every operation rounded once."""
    x = x.float()
    hi = x.half()
    lo = (x - hi.float()).half()
    return hi, lo


def q8_model(x):
    """What a Q8 tensor holds of fp32 x, decoded: hi + e4m3((x - hi) * 2^11) * 2^-11 in float64."""
    x = x.float()
    hi = x.half()
    lo = e4m3_decode(e4m3_encode((x - hi.float()) * 2048.0))
    return hi.double() + lo / 2048.0


def planes(hp):
    """The raw buffer of an HPlanes as [B, G, 2, Hp, Wp, 8] fp16 (a CPU copy)."""
    n = hp.B * hp.G * 2 * hp.Hp * hp.Wp * 8
    return hp.buf[:n].view(hp.B, hp.G, 2, hp.Hp, hp.Wp, 8).cpu().clone()


def second_plane_bytes(pl):
    """[B, G, Hp, Wp, 16] uint8: the second plane of every group as bytes."""
    return pl[:, :, 1].contiguous().view(torch.uint8).view(*pl.shape[:2], *pl.shape[3:5], 16)


def decode(pl, q8, C, H, W):
    """Raw planes -> [B, C, H, W] float64, decoded HERE (not by ssm_hl8_to_f32 / ssm_hq8_to_f32)."""
    B, G = pl.shape[:2]
    hi = pl[:, :, 0].double()                                               # [B, G, Hp, Wp, 8]
    if q8:
        by = second_plane_bytes(pl)
        lo = torch.empty_like(hi)
        for g in range(G):
            lo[:, g] = e4m3_decode(by[:, g | 1, :, :, (g & 1) * 8:(g & 1) * 8 + 8]) / 2048.0
    else:
        lo = pl[:, :, 1].double()
    full = (hi + lo).permute(0, 1, 4, 2, 3).reshape(B, G * 8, pl.shape[3], pl.shape[4])
    return full[:, :C, PADY:PADY + H, PADX:PADX + W]


def encode(x, G, q8, Hp, Wp):
    """fp32 [B, C, H, W] -> the raw planes [B, G, 2, Hp, Wp, 8] fp16 a converter must produce, frame and padding channels zero."""
    B, C, H, W = x.shape
    xp = torch.zeros(B, G * 8, H, W)
    xp[:, :C] = x
    hi, lo = split_hl(xp)
    pl = torch.zeros(B, G, 2, Hp, Wp, 8, dtype=torch.float16)
    put = lambda t: t.view(B, G, 8, H, W).permute(0, 1, 3, 4, 2)          # noqa: E731
    pl[:, :, 0, PADY:PADY + H, PADX:PADX + W] = put(hi)
    if not q8:
        pl[:, :, 1, PADY:PADY + H, PADX:PADX + W] = put(lo)
        return pl
    assert G % 2 == 0
    fx = put(e4m3_encode(xp))                                                # [B, G, H, W, 8] uint8
    fl = put(e4m3_encode((xp - hi.float()) * 2048.0))
    by = torch.zeros(B, G, Hp, Wp, 16, dtype=torch.uint8)
    for g in range(0, G, 2):
        by[:, g, PADY:PADY + H, PADX:PADX + W] = torch.cat([fx[:, g], fx[:, g + 1]], -1)
        by[:, g + 1, PADY:PADY + H, PADX:PADX + W] = torch.cat([fl[:, g], fl[:, g + 1]], -1)
    pl[:, :, 1] = by.view(torch.float16).view(B, G, Hp, Wp, 8)
    return pl


def frame_of(pl, H, W):
    """The planes with the interior zeroed: what must stay zero (both planes)."""
    f = pl.clone()
    f[:, :, :, PADY:PADY + H, PADX:PADX + W] = 0
    return f.view(torch.int16)


def rep_error_bound(absmax, q8):
    """Largest |decoded - x| of an fp32 x with |x| <= absmax written in HL8 / Q8 form, from the formats alone.
    hi = fp16(x): |x - hi| <= ulp16(x) / 2 = 2^(e - 11) for 2^e <= |x| < 2^(e + 1), i.e. <= |x| * 2^-11.
    HL8: lo = fp16(x - hi) rounds a value <= |x| * 2^-11 to 11 bits: error <= |x| * 2^-22 (lo in fp16's normal range: |x| > 2^-3; below it
         lo is a subnormal, spacing 2^-24: error <= 2^-25).
    Q8:  lo8 = e4m3((x - hi) * 2^11): 4 significant bits, error <= |x - hi| * 2^-4 <= |x| * 2^-15 while (x - hi) * 2^11 <= 448, i.e. for
         every |x| < 448 (|x - hi| <= 2^-3 there); e4m3's subnormal spacing 2^-9 adds <= 2^-10 * 2^-11 = 2^-21.
         Above 448 the clamp can lose all of lo: error <= |x| * 2^-11."""
    if not q8:
        return max(absmax * 2.0 ** -22, 2.0 ** -25)
    if absmax < 448:
        return absmax * 2.0 ** -15 + 2.0 ** -21
    return absmax * 2.0 ** -11


# ---- 2. the case table -------------------------------------------------------------------------------------------------------------
MODES = ("split", "fast", "q8")
BARS = {"split": 5e-5, "fast": 2e-2, "q8": 1.5e-4}          # tests/test_hip_conv16.py, tests/test_hip_conv16_q8.py
PLAIN_KINDS = ("H7", "H5", "H3N32", "H3N32D", "H3N64", "H3N128", "H3N128S", "H3N32V", "H3N32W")
UPS_KINDS = ("U3N32", "U3N64", "U3N128", "U3N128S")
# tile sizes from the Cfg16 / CfgUps comments of csrc/ssm_conv16.hip: (BN, TH, TW)
TILE = {"H7": (32, 8, 32), "H5": (64, 8, 64), "H3N32": (32, 8, 64), "H3N32D": (32, 8, 64), "H3N64": (64, 8, 64), "H3N128": (128, 4, 64),
        "H3N128S": (128, 4, 32), "H3N32V": (32, 8, 64), "H3N32W": (32, 8, 64),
        "U3N32": (32, 8, 64), "U3N64": (64, 8, 64), "U3N128": (128, 4, 64), "U3N128S": (128, 4, 32)}


class Case:
    """One problem.  H, W = OUTPUT size (ups: twice the sources').  c2 > 0: a second source; bcast: it has one batch entry read by
    every index; window: the first source is channel groups 2.. of a tensor two groups wider on either side.  cout: (fp32 / HL8, Q8)
    - the Q8 output needs a multiple of 16 - or one number for both; a cout that is no multiple of 8 has the fp32 output only."""

    def __init__(self, kind, tag, k, c1, c2, cout, B, H, W, bcast=False, window=False, slope_half=False):
        self.kind, self.tag, self.k, self.c1, self.c2, self.B, self.H, self.W = kind, tag, k, c1, c2, B, H, W
        self.cout = cout if isinstance(cout, tuple) else (cout, cout)
        self.bcast, self.window, self.slope_half = bcast, window, slope_half
        self.ups = kind.startswith("U")

    def cout_for(self, mode):
        return self.cout[1] if mode == "q8" else self.cout[0]

    @property
    def cin(self):
        return self.c1 + self.c2

    @property
    def id(self):
        return "%s-%s-k%d-%d+%d->%s-%dx%dx%d" % (self.kind, self.tag, self.k, self.c1, self.c2, "%d|%d" % self.cout, self.B, self.H, self.W)

    def pooled(self):
        return not self.ups and self.H % 2 == 0 and self.W % 2 == 0


def _plain(kind, k, deep, cout, wa, wb, ww, below=False, cout5=False):
    """The cases of one plain kind.  cout: a Cout that selects the kind; wa: widths of the small maps (a); wb: the width of (b), one
    whole tile + a ragged one inside the kind's window; ww: an even width inside the window (the pooled cases); below: the kind needs
    Cout <= BN, so "ragged against BN" is BN - 8 | BN - 16 instead of BN + 8 | BN + 16; cout5: the kind takes the bare Cout = 5."""
    bn, th, tw = TILE[kind]
    cs = (128, 144) if deep else (16, 32, 48)
    c0 = cs[0]
    ragged = (bn - 8, bn - 16) if below else (bn + 8, bn + 16)
    out = [Case(kind, "a-h1", k, c0, 0, cout, 1, 1, wa[0]),
           Case(kind, "a-w", k, c0, 0, cout, 2, 3, wa[1]),
           Case(kind, "b-ragged", k, c0, 0, cout, 1, th + 1, wb, slope_half=True),
           Case(kind, "c-cout", k, c0, 0, ragged, 1, th + 2, ww)]
    if cout5:
        out.append(Case(kind, "c-cout5", k, c0, 0, 5, 1, 4, ww))
    out += [Case(kind, "d-cin%d" % c, k, c, 0, cout, 1, 2, ww) for c in cs[1:]]
    if deep:
        out.append(Case(kind, "e-two", k, 64, 80, cout, 2, 4, ww, bcast=True, window=True))
    else:
        out += [Case(kind, "e-two", k, 16, 16, cout, 2, 4, ww, bcast=True), Case(kind, "e-window", k, 32, 16, cout, 2, 2, ww, window=True)]
    return out


def _ups(kind, cout, wa, wb, ww, below=False, cout5=False):
    bn, th, tw = TILE[kind]
    ragged = (bn - 8, bn - 16) if below else (bn + 8, bn + 16)
    out = [Case(kind, "a-1x1" if wa == 2 else "a-h1", 3, 16, 0, cout, 1, 2, wa),
           Case(kind, "b-ragged", 3, 16, 0, cout, 1, th + 2, wb, slope_half=True),
           Case(kind, "c-cout", 3, 16, 0, ragged, 1, 4, ww)]
    if cout5:          # U3N32 also takes every Cout on a narrow map (two cout blocks), and the deep Cin of H3N32D
        out += [Case(kind, "c-cout5", 3, 16, 0, 5, 1, 4, ww), Case(kind, "c-narrow", 3, 16, 0, (40, 48), 2, 6, 34),
                Case(kind, "d-cin144", 3, 144, 0, cout, 1, 2, ww)]
    out += [Case(kind, "d-cin%d" % c, 3, c, 0, cout, 1, 2, ww) for c in (32, 48)]
    out += [Case(kind, "e-two", 3, 16, 16, cout, 2, 4, ww, bcast=True), Case(kind, "e-window", 3, 32, 16, cout, 2, 2, ww, window=True)]
    return out


# W windows (pick16): V / W <= 48; N128S 65..96; N128 49..64 and 97..128; the other 3x3 kinds > 48
PLAIN_CASES = (_plain("H7", 7, False, 32, (1, 1), 33, 34, cout5=True) + _plain("H5", 5, False, 64, (1, 1), 65, 66, cout5=True)
               + _plain("H3N32", 3, False, 32, (49, 50), 65, 66, below=True, cout5=True)
               + _plain("H3N32D", 3, True, 32, (49, 50), 65, 66, below=True, cout5=True)
               + _plain("H3N64", 3, False, 64, (49, 50), 65, 66, below=True) + _plain("H3N128", 3, False, 128, (49, 63), 97, 98)
               + _plain("H3N128S", 3, False, 128, (65, 67), 65, 66)
               + _plain("H3N32V", 3, False, 32, (1, 1), 47, 48, cout5=True) + _plain("H3N32W", 3, True, 32, (1, 1), 47, 48, cout5=True))
UPS_CASES = (_ups("U3N32", 32, 2, 66, 66, below=True, cout5=True) + _ups("U3N64", 64, 50, 66, 66, below=True)
             + _ups("U3N128", 128, 50, 98, 98) + _ups("U3N128S", 128, 66, 66, 68))
ALL_CASES = PLAIN_CASES + UPS_CASES
for _c in ALL_CASES:
    assert _c.B <= 2 and _c.H <= 16 and _c.W <= 128 and _c.cin <= 144, _c.id


# ---- 3. exact-integer data ---------------------------------------------------------------------------------------------------------
def _tern(shape, g, p_zero=1.0 / 3):
    """Values in {-1, 0, 1}."""
    u = torch.rand(shape, generator=g)
    return torch.where(u < p_zero, 0.0, 1.0) * torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)


def _seed(case, mode):
    return 7919 * ALL_CASES.index(case) + MODES.index(mode)


def sources(case, g, make):
    """(a, b or None, cat): the two sources (b with one batch entry when bcast) and the tensor the convolution sees.  The sources of a
    fused-upsample case have half the output size."""
    h, w = (case.H // 2, case.W // 2) if case.ups else (case.H, case.W)
    a = make((case.B, case.c1, h, w), g)
    b = make((1 if case.bcast else case.B, case.c2, h, w), g) if case.c2 else None
    return a, b, (a if b is None else torch.cat([a, b.expand(case.B, -1, -1, -1)], 1))


def exact_inputs(case, mode):
    """Exact-integer problem: activations in {-1, 0, 1} (fused upsample: {-16, 0, 16}, so the bilinear weights (9, 3, 3, 1) / 16 give
    integers in [-16, 16]), filters in {-1, 0, 1} (PackedConv16 then scales by 8: exact in fp16 and e4m3), integer bias in [-3, 3]."""
    g = torch.Generator().manual_seed(_seed(case, mode))
    amp = 16.0 if case.ups else 1.0
    a, b, cat = sources(case, g, lambda s, gg: _tern(s, gg) * amp)
    cout = case.cout_for(mode)
    w = _tern((cout, case.cin, case.k, case.k), g)
    bias = torch.randint(-3, 4, (cout,), generator=g).float()
    return a, b, cat, w, bias


def random_inputs(case, mode):
    g = torch.Generator().manual_seed(_seed(case, mode) + 3)
    a, b, cat = sources(case, g, lambda s, gg: torch.randn(s, generator=gg))
    cout = case.cout_for(mode)
    w = torch.randn(cout, case.cin, case.k, case.k, generator=g) / (case.cin * case.k * case.k) ** 0.5
    bias = torch.randn(cout, generator=g) * 0.1
    return a, b, cat, w, bias


def upsample2x_f64(x):
    """F.upsample(x, scale_factor=2, mode='bilinear') (align_corners=False) in float64."""
    return F.interpolate(x.to(F64), scale_factor=2, mode="bilinear", align_corners=False)


def conv_exact(case, cat, w, bias, lrelu=False, slope=0.5):
    """The convolution of an exact-integer problem in float64 (every value an integer or, after the slope, a half-integer: float64 holds
    them exactly, as int64 would), and its 2x2 mean.  Returns (y, pooled or None)."""
    x = upsample2x_f64(cat) if case.ups else cat.to(F64)
    y = F.conv2d(x, w.to(F64), bias.to(F64), padding=case.k // 2)
    pre = y
    if lrelu:
        y = torch.where(y > 0, y, y * slope)
    return y, (F.avg_pool2d(y, 2) if case.pooled() else None), float(pre.abs().max())
