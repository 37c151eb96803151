"""No-GPU checks of ssm_amd.video: the YUV4MPEG2 reader / writer, the output order of the streamed loop, and the two numpy float32
yardsticks (yuv_to_frames_host, frames_to_yuv_host) that the HIP kernels of csrc/ssm_video.hip are held to bit for bit in
tests/test_hip_video.py.  The yardsticks themselves are held here to known colours and to an independent float64 evaluation of the
same formulas (interpolation and decimation written as matrices from the sample positions, constants straight from Kr / Kb).

Bars of the float64 comparison.
  Ingest, |fp32 - fp64| <= 1e-5 in normalised units.  u = 2^-24.  The chroma stencils (weights 1/4, 1/2, 3/4, 1 on 8-bit codes)
  are exact in fp32.  y' = (Y - off) ys carries the rounding of the constant and of the product: 2u |y'|, |y'| <= 297; likewise cb, cr
  with |c| <= 146.  A product k c carries 4u |k c| (constant, c's two, its own), |k c| <= 1.86 * 146 < 272; G has two.  Every sum rounds
  once more at u |sum|, |sum| <= 570.  Worst case G: 2*297u + 2*4*272u + 2*570u = 3910u < 2^12 u = 2.5e-4 of a code.  The clamp does not
  expand it.  / 255 (u relative), - mean (the constant's and the difference's rounding: 2u absolute at most), / std (constant and
  quotient: 2u relative of |n| <= 2.7) with std >= 0.224 give 2.5e-4 / 255 / 0.224 + 2u / 0.224 + 2u * 2.7 + u * 2.7 < 5.4e-6; the bar
  is that bound rounded up to 1e-5.
  Egress, codes EQUAL wherever the float64 value before rounding lies further than 1e-3 from a tie (k + 1/2): with inputs that reach
  codes of magnitude < 600 the fp32 value carries < 600 * 16u = 6e-4.  The samples left out may be 1 % of the set at most; the share
  observed on this seeded set is 0.17-0.39 % per case for 4:2:0 and for limited range, 0.85-0.87 % for full-range 4:4:4 (a uniform
  fraction would give 0.2 %)."""
import io
import itertools

import numpy as np
import pytest

from ssm_amd import video as V
from ssm_amd.weights import IMAGENET_MEAN, IMAGENET_STD

SIZES = ((46, 70), (45, 71))
CASES = list(itertools.product((V.CENTRED, V.COSITED, V.C444), (V.BT601, V.BT709), (V.LIMITED, V.FULL), SIZES))


def stream_of(n, w=6, h=4, chroma="420jpeg", head_extra="", cut=0):
    fb = V.frame_bytes(h, w, V.CHROMA_TAGS.get(chroma, 0))
    body = b"".join(b"FRAME\n" + bytes([(7 * i + j) % 256 for j in range(fb)]) for i in range(n))
    data = ("YUV4MPEG2 W%d H%d F30000:1001 Ip A1:1 C%s%s\n" % (w, h, chroma, head_extra)).encode() + body
    return io.BytesIO(data[:len(data) - cut])


# ---- container ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chroma,siting", [("420", V.CENTRED), ("420jpeg", V.CENTRED), ("420mpeg2", V.COSITED), ("444", V.C444)])
@pytest.mark.parametrize("crange", [None, V.LIMITED, V.FULL])
def test_header_round_trip(chroma, siting, crange):
    buf = io.BytesIO()
    w = V.Y4MWriter(buf, 7, 5, rate=(30000, 1001), aspect=(4, 3), chroma=chroma, color_range=crange, xtags=("YSCSS=420JPEG",))
    frames = [bytes([(i * 31 + j) % 256 for j in range(w.frame_bytes)]) for i in range(3)]
    for f in frames:
        w.write_frame(f)
    w.close()
    buf.seek(0)
    r = V.Y4MReader(buf)
    assert (r.width, r.height, r.rate, r.aspect, r.chroma, r.siting, r.interlace) == (7, 5, (30000, 1001), (4, 3), chroma, siting, "p")
    assert r.color_range == crange and "YSCSS=420JPEG" in r.xtags
    assert ("COLORRANGE=" + {V.LIMITED: "LIMITED", V.FULL: "FULL"}[crange] in r.xtags) if crange is not None else not any("COLORRANGE" in x for x in r.xtags)
    got = bytearray(r.frame_bytes)
    for f in frames:
        assert r.read_frame_into(got) and bytes(got) == f
    assert not r.read_frame_into(got) and r.frames_read == 3
    # a writer made like the reader emits the same header again (the rate overridden)
    buf2 = io.BytesIO()
    V.Y4MWriter.like(buf2, r, rate=(240000, 1001)).close()
    assert buf2.getvalue().decode().split()[1:4] == ["W7", "H5", "F240000:1001"]
    assert V.Y4MReader(io.BytesIO(buf2.getvalue())).color_range == crange


def test_header_defaults_and_frame_parameters():
    r = V.Y4MReader(io.BytesIO(b"YUV4MPEG2 W4 H2\nFRAME Ip\n" + bytes(12)))
    assert (r.chroma, r.siting, r.rate, r.color_range) == ("420jpeg", V.CENTRED, (25, 1), None)
    assert r.read_frame_into(bytearray(12))
    assert V.Y4MReader(stream_of(1, head_extra=" XCOLORRANGE=FULL")).color_range == V.FULL


@pytest.mark.parametrize("tag", ["422", "mono", "420paldv", "420p10", "420p12", "420p16", "422p10", "444p10", "444p16", "444alpha", "411"])
def test_refused_colour_spaces_are_named(tag):
    with pytest.raises(V.Y4MError, match="C" + tag):
        V.Y4MReader(stream_of(1, chroma=tag))
    with pytest.raises(V.Y4MError, match="C" + tag):
        V.Y4MWriter(io.BytesIO(), 4, 4, chroma=tag)


@pytest.mark.parametrize("tag", ["t", "b", "m"])
def test_interlaced_input_is_refused(tag):
    data = stream_of(1).getvalue().replace(b" Ip ", (" I%s " % tag).encode())
    with pytest.raises(V.Y4MError, match="I" + tag):
        V.Y4MReader(io.BytesIO(data))


def test_truncated_streams_raise():
    with pytest.raises(V.Y4MError, match="YUV4MPEG2"):
        V.Y4MReader(io.BytesIO(b"RIFF....AVI "))
    with pytest.raises(V.Y4MError):
        V.Y4MReader(io.BytesIO(b"YUV4MPEG2 W4 H4"))                 # header cut before its newline
    r = V.Y4MReader(stream_of(3, cut=5))
    buf = bytearray(r.frame_bytes)
    assert r.read_frame_into(buf) and r.read_frame_into(buf)
    with pytest.raises(V.Y4MError, match="frame 2 is truncated"):
        r.read_frame_into(buf)
    r = V.Y4MReader(stream_of(2, cut=V.frame_bytes(4, 6, 0) + 3))    # cut inside the second FRAME line
    assert r.read_frame_into(buf)
    with pytest.raises(V.Y4MError, match="FRAME"):
        r.read_frame_into(buf)
    with pytest.raises(ValueError):
        V.Y4MWriter(io.BytesIO(), 4, 4).write_frame(bytes(5))


# ---- order of the output -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 9])
@pytest.mark.parametrize("rate", [2, 8])
@pytest.mark.parametrize("pb", [1, 2, 4])
def test_frame_counts_and_order(n, rate, pb):
    order = V.clip_order(n, rate, pb)
    assert len(order) == (n - 1) * rate + 1
    assert order == [(i // rate, i % rate) for i in range((n - 1) * rate + 1)]          # time order: input i, then its rate - 1 steps
    assert [o for o in order if o[1] == 0] == [(i, 0) for i in range(n)]                 # every input frame once, in order
    for slowmo in (False, True):
        num, den = V.output_rate((30000, 1001), rate, slowmo)
        assert den == 1001 and num == (30000 if slowmo else 30000 * rate)
        # duration: the same with the multiplied rate, `rate` times longer (minus the open end) in slow motion
        assert abs(len(order) * den / num - ((n - 1) * (rate if slowmo else 1) + (1 if slowmo else 1 / rate)) * 1001 / 30000) < 1e-9


def test_pass_order_is_interpolated_frames_then_the_right_frame():
    assert list(V.pass_order(2, 3)) == [("interp", 0), ("interp", 1), ("interp", 2), ("orig", 0),
                                        ("interp", 3), ("interp", 4), ("interp", 5), ("orig", 1)]


# ---- known colours -----------------------------------------------------------------------------------------------------------------
def const_frame(y, u, v, h, w, siting):
    ch, cw = V.chroma_dims(h, w, siting)
    return np.concatenate([np.full(h * w, y, np.uint8), np.full(ch * cw, u, np.uint8), np.full(ch * cw, v, np.uint8)])[None]


@pytest.mark.parametrize("siting", [V.CENTRED, V.COSITED, V.C444])
@pytest.mark.parametrize("matrix", [V.BT601, V.BT709])
def test_black_and_white_in_both_ranges(siting, matrix):
    h, w = 6, 10
    (hp, wp), (top, left) = ((32, 32), (13, 11))
    mean, std = np.float32(IMAGENET_MEAN), np.float32(IMAGENET_STD)
    black = (np.float32(0.0) / np.float32(255.0) - mean) / std
    white = (np.float32(255.0) / np.float32(255.0) - mean) / std
    for crange, lo, hi in ((V.LIMITED, 16, 235), (V.FULL, 0, 255)):
        for code, want in ((lo, black), (hi, white)):
            x = V.yuv_to_frames_host(const_frame(code, 128, 128, h, w, siting), h, w, siting, matrix, crange)
            assert x.shape == (1, 3, hp, wp) and x.dtype == np.float32
            inner = x[0, :, top:top + h, left:left + w]
            # (235 - 16) * fp32(255/219) is 255 to within an fp32 rounding; the normalised value to within two
            assert np.abs(inner - want[:, None, None]).max() <= 4e-7 * np.abs(want).max(), (crange, code)
            if code == lo:
                assert np.array_equal(inner, np.broadcast_to(want[:, None, None], inner.shape))          # black is exact
            assert np.array_equal(x[0, :, 0, 0], black)                                                  # pad ring: black before normalisation
            back = V.frames_to_yuv_host(x, h, w, siting, matrix, crange)
            assert np.array_equal(back, const_frame(code, 128, 128, h, w, siting))
    x = V.yuv_to_frames_host(const_frame(16, 128, 128, h, w, siting), h, w, siting, matrix, V.LIMITED, pad_before_norm=False)
    assert float(np.abs(x[0, :, 0, 0]).max()) == 0.0


@pytest.mark.parametrize("matrix", [V.BT601, V.BT709])
def test_grey_ramp_is_exact_through_444(matrix):
    """All 256 Y codes survive ingest -> egress in full range; in limited range the 220 legal codes 16..235 do, and the codes outside
    them, which the ingest clamps to black / white, come back as 16 / 235."""
    h, w = 8, 32
    ramp = np.arange(256, dtype=np.uint8)
    frame = np.concatenate([ramp, np.full(2 * h * w, 128, np.uint8)])[None]
    full = V.frames_to_yuv_host(V.yuv_to_frames_host(frame, h, w, V.C444, matrix, V.FULL), h, w, V.C444, matrix, V.FULL)
    assert np.array_equal(full, frame)
    lim = V.frames_to_yuv_host(V.yuv_to_frames_host(frame, h, w, V.C444, matrix, V.LIMITED), h, w, V.C444, matrix, V.LIMITED)
    assert np.array_equal(lim[0, :256], np.clip(ramp, 16, 235)) and np.array_equal(lim[0, 256:], frame[0, 256:])


def test_primaries_land_where_the_matrix_says():
    """Full-range BT.601 red (Y, Cb, Cr) = (76, 85, 255) within a code: the well-known JPEG triple."""
    x = np.zeros((1, 3, 32, 32), np.float32)
    mean, std = np.float32(IMAGENET_MEAN), np.float32(IMAGENET_STD)
    for p, v in enumerate((1.0, 0.0, 0.0)):
        x[0, p] = (np.float32(v) - mean[p]) / std[p]
    out = V.frames_to_yuv_host(x, 4, 4, V.C444, V.BT601, V.FULL)[0]
    assert abs(int(out[0]) - 76) <= 1 and abs(int(out[16]) - 85) <= 1 and int(out[32]) == 255


# ---- float64 evaluation of the same formulas ---------------------------------------------------------------------------------------
def consts64(matrix, crange):
    kr, kb = ((0.299, 0.114), (0.2126, 0.0722))[matrix]
    lim = crange == V.LIMITED
    return dict(kr=kr, kb=kb, kg=1.0 - kr - kb, ys=255.0 / 219.0 if lim else 1.0, cs=255.0 / 224.0 if lim else 1.0,
                yoff=16.0 if lim else 0.0, ylo=16.0 if lim else 0.0, yhi=235.0 if lim else 255.0, clo=16.0 if lim else 0.0,
                chi=240.0 if lim else 255.0)


def interp_matrix(n_out, n_in, centred):
    """[n_out, n_in] float64: linear interpolation at the position of output sample x in input units, x/2 - 1/4 (input samples centred
    between two outputs) or x/2 (co-sited with the even outputs), indices clamped to the input."""
    m = np.zeros((n_out, n_in))
    for x in range(n_out):
        pos = x / 2.0 - (0.25 if centred else 0.0)
        i0 = int(np.floor(pos))
        f = pos - i0
        m[x, min(max(i0, 0), n_in - 1)] += 1.0 - f
        m[x, min(max(i0 + 1, 0), n_in - 1)] += f
    return m


def decim_matrix(n_out, n_in, taps):
    """[n_out, n_in] float64: output c = sum_k taps[k] * input[clamp(2c + offset_k)]; taps = {offset: weight}."""
    m = np.zeros((n_out, n_in))
    for c in range(n_out):
        for off, wgt in taps.items():
            m[c, min(max(2 * c + off, 0), n_in - 1)] += wgt
    return m


def ingest64(payload, h, w, siting, matrix, crange, pad_before_norm):
    k = consts64(matrix, crange)
    y, u, v = [p.astype(np.float64) for p in V.split_planes(payload, h, w, siting)]
    if siting != V.C444:
        mv, mh = interp_matrix(h, u.shape[1], True), interp_matrix(w, u.shape[2], siting == V.CENTRED)
        u, v = mv @ u @ mh.T, mv @ v @ mh.T
    yl, cb, cr = (y - k["yoff"]) * k["ys"], (u - 128.0) * k["cs"], (v - 128.0) * k["cs"]
    r = yl + 2.0 * (1.0 - k["kr"]) * cr
    b = yl + 2.0 * (1.0 - k["kb"]) * cb
    g = (yl - k["kr"] * r - k["kb"] * b) / k["kg"]          # from Y = Kr R + Kg G + Kb B
    hp, wp = -(-h // 32) * 32, -(-w // 32) * 32
    top, left = (hp - h) // 2, (wp - w) // 2
    out = np.zeros((payload.shape[0], 3, hp, wp))
    for p, c in enumerate((r, g, b)):
        if pad_before_norm:
            out[:, p] = (0.0 - IMAGENET_MEAN[p]) / IMAGENET_STD[p]
        out[:, p, top:top + h, left:left + w] = (np.clip(c, 0.0, 255.0) / 255.0 - IMAGENET_MEAN[p]) / IMAGENET_STD[p]
    return out


def egress64(x, h, w, siting, matrix, crange):
    """float64 values BEFORE rounding, and the codes: ([N, frame_bytes] float64, [N, frame_bytes] uint8)."""
    k = consts64(matrix, crange)
    hp, wp = x.shape[2:]
    top, left = (hp - h) // 2, (wp - w) // 2
    r, g, b = [(x[:, p, top:top + h, left:left + w].astype(np.float64) * IMAGENET_STD[p] + IMAGENET_MEAN[p]) * 255.0 for p in range(3)]
    yf = k["kr"] * r + k["kg"] * g + k["kb"] * b
    cb, cr = (b - yf) / (2.0 * (1.0 - k["kb"])), (r - yf) / (2.0 * (1.0 - k["kr"]))
    if siting != V.C444:
        ch, cw = V.chroma_dims(h, w, siting)
        mv = decim_matrix(ch, h, {0: 0.5, 1: 0.5})
        mh = decim_matrix(cw, w, {0: 0.5, 1: 0.5} if siting == V.CENTRED else {-1: 0.25, 0: 0.5, 1: 0.25})
        cb, cr = mv @ cb @ mh.T, mv @ cr @ mh.T
    n = x.shape[0]
    pre = np.concatenate([(yf / k["ys"] + k["yoff"]).reshape(n, -1), (cb / k["cs"] + 128.0).reshape(n, -1), (cr / k["cs"] + 128.0).reshape(n, -1)], 1)
    lo = np.concatenate([np.full(h * w, k["ylo"]), np.full(pre.shape[1] - h * w, k["clo"])])
    hi = np.concatenate([np.full(h * w, k["yhi"]), np.full(pre.shape[1] - h * w, k["chi"])])
    return pre, np.clip(np.rint(pre), lo, hi).astype(np.uint8)


def seeded_payload(n, h, w, siting, seed):
    rng = np.random.RandomState(seed)
    return rng.randint(0, 256, size=(n, V.frame_bytes(h, w, siting))).astype(np.uint8)


def seeded_planes(n, h, w, seed):
    """Normalised planes whose denormalised values cover [-0.4, 1.4]: both saturation bounds of every plane are reached."""
    rng = np.random.RandomState(seed)
    hp, wp = -(-h // 32) * 32, -(-w // 32) * 32
    v = rng.uniform(-0.4, 1.4, size=(n, 3, hp, wp))
    # 4 x 4 patches of the extreme colours (inside every crop used here): every plane reaches both of its bounds whatever the draw
    for i, rgb in enumerate(((-0.4, -0.4, 1.4), (1.4, 1.4, -0.4), (1.4, -0.4, -0.4), (-0.4, 1.4, 1.4), (1.4, 1.4, 1.4), (-0.4, -0.4, -0.4))):
        v[:, :, hp // 2 - 2:hp // 2 + 2, wp // 2 - 12 + 4 * i:wp // 2 - 8 + 4 * i] = np.asarray(rgb)[None, :, None, None]
    return ((v - np.asarray(IMAGENET_MEAN)[None, :, None, None]) / np.asarray(IMAGENET_STD)[None, :, None, None]).astype(np.float32)


INGEST_TOL = 1e-5          # derived in the module docstring
TIE_GUARD, TIE_SHARE = 1e-3, 0.01


@pytest.mark.parametrize("siting,matrix,crange,size", CASES)
def test_ingest_yardstick_against_float64(siting, matrix, crange, size):
    h, w = size
    payload = seeded_payload(2, h, w, siting, 100 + siting)
    for pbn in (True, False):
        got = V.yuv_to_frames_host(payload, h, w, siting, matrix, crange, pad_before_norm=pbn)
        want = ingest64(payload, h, w, siting, matrix, crange, pbn)
        assert got.dtype == np.float32 and got.shape == want.shape
        err = float(np.abs(got.astype(np.float64) - want).max())
        print("ingest siting %d matrix %d range %d %dx%d pbn %d: max |fp32 - fp64| = %.3e" % (siting, matrix, crange, h, w, pbn, err))
        assert err <= INGEST_TOL, err


@pytest.mark.parametrize("siting,matrix,crange,size", CASES)
def test_egress_yardstick_against_float64(siting, matrix, crange, size):
    h, w = size
    x = seeded_planes(2, h, w, 200 + siting)
    got = V.frames_to_yuv_host(x, h, w, siting, matrix, crange)
    pre, want = egress64(x, h, w, siting, matrix, crange)
    assert got.shape == want.shape and got.dtype == np.uint8
    near_tie = np.abs(pre - np.floor(pre) - 0.5) < TIE_GUARD
    share = float(near_tie.mean())
    print("egress siting %d matrix %d range %d %dx%d: %.3f %% within %.0e of a tie, %d codes differ outside them"
          % (siting, matrix, crange, h, w, 100 * share, TIE_GUARD, int((got != want)[~near_tie].sum())))
    assert share <= TIE_SHARE, share
    assert np.array_equal(got[~near_tie], want[~near_tie])
    lo, hi = (16, 235) if crange == V.LIMITED else (0, 255)
    assert got[:, :h * w].min() == lo and got[:, :h * w].max() == hi          # both saturation bounds are reached
    assert got[:, h * w:].min() == lo and got[:, h * w:].max() == (240 if crange == V.LIMITED else 255)


def test_table_is_float64_rounded_once():
    t = V.yuv_table()
    assert t.shape == (2, 2, V.YUV_ROW) and t.dtype == np.float32
    for m, (kr, kb) in enumerate(((0.299, 0.114), (0.2126, 0.0722))):
        kg = 1.0 - kr - kb
        assert t[m, 0, 0] == np.float32(kr) and t[m, 0, 1] == np.float32(kg) and t[m, 0, 2] == np.float32(kb)
        assert t[m, 0, 4] == np.float32(2.0 * (1.0 - kb) * kb / kg) and t[m, 1, 9] == 1.0 and t[m, 0, 9] == np.float32(255.0 / 219.0)
        assert list(t[m, 0, 13:19]) == [16, 128, 16, 235, 16, 240] and list(t[m, 1, 13:19]) == [0, 128, 0, 255, 0, 255]
    assert V.default_matrix(720) == V.BT709 and V.default_matrix(719) == V.BT601
