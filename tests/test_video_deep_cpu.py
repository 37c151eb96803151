"""No-GPU checks of the 4:2:2 and 9- to 16-bit formats of ssm_amd.video: the constant table of a bit depth, the extended YUV4MPEG2
reader / writer, and the two numpy float32 yardsticks (yuv_to_frames_host, frames_to_yuv_host with layout 3 and bits > 8) that the HIP
kernels are held to bit for bit in tests/test_hip_video_deep.py.  The yardsticks are held here to an exact round trip and to the float64
evaluation of tests/video_deep_clips.py, written from the defining formulas and not through yuv_table.

Bars of the float64 comparison, u = 2^-24, s = 2^(bits - 8).  The kernels work in 0 .. 255 units whatever the depth, so the magnitudes are
those of tests/test_video_cpu.py and only what depends on the size of a code changes.
  Ingest, |fp32 - fp64| <= 1e-5 in normalised units, the bar of the 8-bit test, by its derivation: the chroma stencils stay exact - a
  16-bit code times 1/4, 1/2 or 3/4 and the sum of two such has at most 18 bits, the vertical step of 4:2:0 makes it 20, the difference
  from the offset no more, all below fp32's 24; the two scale factors are again float64 constants rounded once.  From there on the values
  are those of the 8-bit case (|y'| <= 297, |c| <= 146 in 0 .. 255 units) and the count of roundings is the same: 3910 u of a 0 .. 255
  unit before the clamp, < 5.4e-6 after normalisation.  Worst value seen on these seeded sets: 9.8e-7 (10 and 16 bits alike).
  Egress, codes EQUAL wherever the float64 value before rounding lies further than GUARD = s * 2^-11 codes from a tie.  Count, for inputs
  whose denormalised values lie in [-0.4, 1.4]: v = x std + mean carries 2u |x std| + u |mean| + u |v| <= 5.7u (|x std| <= 1.9); times
  255: 255 * 5.7u + u * 357 < 1810u.  Yf: that, weighted by weights that sum to 1, plus two roundings (constant, product) on each of
  three products and two sums, together bounded by 4u * 357: < 3240u.  Cb = (B - Yf) cbs: 1810u + 3240u + u |B - Yf| (<= 430) +
  2u |Cb| (<= 230): < 5940u.  The chroma filter's four terms and final quarter are exact but for three sums at u * 230 each: < 6630u.
  The code C ics + coff: ics <= 1.004 s, its constant and the product 2u * 230 s, the sum u |code| with |code| <= 358 s:
  (6630 * 1.004 + 460 + 358) s u < 7500 s u < 8192 s u = s * 2^-11 codes - 1.95e-3 of a code at 10 bits, 0.125 at 16.  fp32 carries 24
  bits and a 16-bit code with its headroom needs 17 of them: an eighth of a code is what the pipeline's precision is at that depth.
  The share of samples inside the guard is capped at 1 %.  At 10 bits the inputs are uniform draws, as in the 8-bit test, and the share
  seen is 0.28-0.57 % per case (a uniform fraction would give 0.39 %).  At 16 bits uniform draws would put 25 % of the samples inside
  the guard, so those inputs are built to stay clear of ties in exact arithmetic (video_deep_clips.ramp_payload: legal in-gamut
  codes, chroma planes that are ramps which every layout's filters interpolate and decimate to whole numbers, ingested in float64): the
  values before rounding are whole numbers but for the fp32 rounding of the planes, the share seen is 0 %, every code is compared, and
  the luma codes (and a constant chroma plane) must be the payload's own - a chroma ramp comes back as itself away from the plane's
  edges only, where the clamped indices bend it."""
import io
import itertools
import os
import sys

import numpy as np
import pytest

from ssm_amd import video as V

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import video_deep_clips as D  # noqa: E402

BITS = (8, 9, 10, 12, 14, 16)
INGEST_TOL = 1e-5
TIE_SHARE = 0.01


def tie_guard(bits):
    return 2.0 ** (bits - 8) * 2.0 ** -11


# ---- the table ----------------------------------------------------------------------------------------------------------------------
def test_table_of_8_bits_is_the_table_as_it_was():
    assert np.array_equal(V.yuv_table(8).view(np.uint32), V.yuv_table().view(np.uint32))
    kr, kb = 0.2126, 0.0722
    t = V.yuv_table()
    assert t[1, 0, 9] == np.float32(255.0 / 219.0) and t[1, 0, 12] == np.float32(224.0 / 255.0) and t[1, 1, 9] == 1.0 and t[1, 1, 11] == 1.0
    assert t[1, 0, 3] == np.float32(2.0 * (1.0 - kr)) and t[1, 0, 7] == np.float32(1.0 / (2.0 * (1.0 - kb)))


@pytest.mark.parametrize("bits", BITS)
def test_bounds_and_scales_of_every_depth(bits):
    t = V.yuv_table(bits)
    s, peak = 2 ** (bits - 8), 2 ** bits - 1
    assert t.shape == (2, 2, V.YUV_ROW) and t.dtype == np.float32
    for m in (0, 1):
        assert list(t[m, 0, 13:19]) == [16 * s, 128 * s, 16 * s, 235 * s, 16 * s, 240 * s]
        assert list(t[m, 1, 13:19]) == [0, 128 * s, 0, peak, 0, peak]
        assert t[m, 0, 9] == np.float32(255.0 / (219.0 * s)) and t[m, 0, 10] == np.float32(255.0 / (224.0 * s))
        assert t[m, 0, 11] == np.float32(219.0 * s / 255.0) and t[m, 0, 12] == np.float32(224.0 * s / 255.0)
        assert t[m, 1, 9] == t[m, 1, 10] == np.float32(255.0 / peak) and t[m, 1, 11] == t[m, 1, 12] == np.float32(peak / 255.0)
        assert np.array_equal(t[m, :, :9], V.yuv_table(8)[m, :, :9])          # the matrix does not depend on the depth
    assert V._table_ptr(bits) is V._table_ptr(bits) and (bits == 8 or V._table_ptr(bits) is not V._table_ptr(8))


@pytest.mark.parametrize("bits", [7, 17, 0, 10.5, True])
def test_depths_outside_8_to_16_are_refused(bits):
    with pytest.raises(ValueError, match="8 to 16"):
        V.yuv_table(bits)


# ---- container ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,layout,bits,hand", [("422", V.C422, 8, 7 * 5 + 2 * 5 * 4), ("420p10", V.CENTRED, 10, 2 * (7 * 5 + 2 * 3 * 4)),
                                                  ("422p10", V.C422, 10, 2 * (7 * 5 + 2 * 5 * 4)), ("444p12", V.C444, 12, 2 * 3 * 7 * 5),
                                                  ("444p16", V.C444, 16, 2 * 3 * 7 * 5)])
def test_extended_header_round_trip(tag, layout, bits, hand):
    buf = io.BytesIO()
    w = V.Y4MWriter(buf, 7, 5, rate=(30000, 1001), aspect=(4, 3), chroma=tag, color_range=V.FULL, extended=True)
    assert (w.siting, w.bits, w.sample_bytes, w.frame_bytes) == (layout, bits, 1 if bits == 8 else 2, hand)
    assert V.frame_bytes(5, 7, layout, bits) == hand and V.chroma_dims(5, 7, layout, bits) == D.dims(5, 7, layout)
    frames = [bytes([(i * 31 + j) % 256 for j in range(hand)]) for i in range(3)]
    for f in frames:
        w.write_frame(f)
    w.close()
    r = V.Y4MReader(io.BytesIO(buf.getvalue()), extended=True)
    assert (r.width, r.height, r.rate, r.chroma, r.siting, r.bits, r.sample_bytes, r.frame_bytes) == \
        (7, 5, (30000, 1001), tag, layout, bits, 1 if bits == 8 else 2, hand)
    if layout == V.C422:
        assert V.chroma_dims(5, 7, layout) == (5, 4)          # odd width: ceil(7 / 2) columns, every row
    got = bytearray(hand)
    for f in frames:
        assert r.read_frame_into(got) and bytes(got) == f
    assert not r.read_frame_into(got)
    buf2 = io.BytesIO()
    like = V.Y4MWriter.like(buf2, r, rate=(60, 1))
    like.close()
    assert like.extended and (like.chroma, like.bits, like.frame_bytes) == (tag, bits, hand)
    assert "C" + tag in buf2.getvalue().decode().split() and V.Y4MReader(io.BytesIO(buf2.getvalue()), extended=True).chroma == tag


def test_a_sample_is_a_little_endian_word():
    frame = bytes([0x34, 0x02, 0xff, 0x03, 0x00, 0x00, 0x01, 0x00]) + bytes(range(16))
    r = V.Y4MReader(io.BytesIO(b"YUV4MPEG2 W2 H2 C444p10\nFRAME\n" + frame), extended=True)
    buf = np.empty(r.frame_bytes, np.uint8)
    assert r.frame_bytes == 24 and r.read_frame_into(buf)
    y, u, v = V.split_planes(buf[None], 2, 2, r.siting, r.bits)
    assert y.dtype.itemsize == 2 and y.shape == (1, 2, 2) and u.shape == v.shape == (1, 2, 2)
    assert y[0, 0, 0] == 0x0234 and y[0].tolist() == [[0x0234, 0x03ff], [0, 1]] and u[0, 0, 0] == 0x0100 and v[0, 1, 1] == 0x0f0e
    y8, _, _ = V.split_planes(buf[None, :12], 2, 2, V.C444)          # three or four positional arguments: as before
    assert y8.dtype == np.uint8 and y8[0, 0].tolist() == [0x34, 0x02]


@pytest.mark.parametrize("tag", ["mono", "411", "444alpha", "420paldv", "420p11"])
def test_tags_outside_the_extended_set_are_refused_by_name(tag):
    data = ("YUV4MPEG2 W4 H4 C%s\n" % tag).encode()
    for make in (lambda: V.Y4MReader(io.BytesIO(data), extended=True), lambda: V.Y4MWriter(io.BytesIO(), 4, 4, chroma=tag, extended=True)):
        with pytest.raises(V.Y4MError, match="C" + tag + " .*C422pB"):
            make()


def test_without_the_flag_nothing_new_is_taken():
    for tag in ("422", "422p10", "444p16"):
        with pytest.raises(V.Y4MError, match="C" + tag + r" is not supported \(8-bit C420, C420jpeg, C420mpeg2 and C444 are\)"):
            V.Y4MReader(io.BytesIO(("YUV4MPEG2 W4 H4 C%s\n" % tag).encode()))
    r = V.Y4MReader(io.BytesIO(b"YUV4MPEG2 W4 H2\n"))
    assert (r.bits, r.sample_bytes, r.extended) == (8, 1, False)
    with pytest.raises(V.Y4MError, match="It"):
        V.Y4MReader(io.BytesIO(b"YUV4MPEG2 W4 H4 It C422p10\n"), extended=True)


# ---- the round trip through the yardsticks alone is exact ---------------------------------------------------------------------------
@pytest.mark.parametrize("bits,matrix,crange", list(itertools.product((8, 10, 12, 16), (V.BT601, V.BT709), (V.LIMITED, V.FULL))))
def test_legal_greys_and_in_gamut_colours_come_back_exactly(bits, matrix, crange):
    k = D.consts64(matrix, crange, bits)
    grey = np.arange(int(k["ylo"]), int(k["yhi"]) + 1)
    w = 512
    h = -(-grey.size // w)
    y = np.concatenate([grey, np.full(h * w - grey.size, grey[-1])]).reshape(1, h, w)
    mid = np.full((1, h, w), int(k["coff"]))
    ramp = D.payload_of(y, mid, mid, bits)
    back = V.frames_to_yuv_host(V.yuv_to_frames_host(ramp, h, w, V.C444, matrix, crange, bits=bits), h, w, V.C444, matrix, crange, bits=bits)
    assert back.dtype == np.uint8 and np.array_equal(back, ramp), "every legal grey code survives ingest -> egress"
    colours, m = D.ingamut_pixels(200000, matrix, crange, bits, 900 + bits)
    assert m > 20000
    back = V.frames_to_yuv_host(V.yuv_to_frames_host(colours, 1, m, V.C444, matrix, crange, bits=bits), 1, m, V.C444, matrix, crange, bits=bits)
    bad = int((back.view("<u2" if bits > 8 else np.uint8) != colours.view("<u2" if bits > 8 else np.uint8)).sum())
    print("bits %d matrix %d range %d: %d in-gamut colours, %d samples differ" % (bits, matrix, crange, m, bad))
    assert bad == 0


# ---- float64 evaluation of the defining formulas ------------------------------------------------------------------------------------
F64_CASES = list(itertools.product((10, 16), (V.CENTRED, V.COSITED, V.C444, V.C422), (V.BT601, V.BT709), (V.LIMITED, V.FULL)))
H, W = 45, 71


@pytest.mark.parametrize("bits,layout,matrix,crange", F64_CASES)
def test_ingest_yardstick_against_float64(bits, layout, matrix, crange):
    payload = D.seeded_payload(2, H, W, layout, bits, 100 + layout + bits)
    for pbn in (True, False):
        got = V.yuv_to_frames_host(payload, H, W, layout, matrix, crange, pad_before_norm=pbn, bits=bits)
        want = D.ingest64(payload, H, W, layout, matrix, crange, bits, pbn)
        assert got.dtype == np.float32 and got.shape == want.shape
        err = float(np.abs(got.astype(np.float64) - want).max())
        print("ingest bits %d layout %d matrix %d range %d pbn %d: max |fp32 - fp64| = %.3e" % (bits, layout, matrix, crange, pbn, err))
        assert err <= INGEST_TOL, err


@pytest.mark.parametrize("bits,layout,matrix,crange", F64_CASES)
def test_egress_yardstick_against_float64(bits, layout, matrix, crange):
    k = D.consts64(matrix, crange, bits)
    if bits == 16:
        payload = D.ramp_payload(H, W, layout, crange, bits, 300 + layout)
        x = D.ingest64(payload, H, W, layout, matrix, crange, bits).astype(np.float32)
    else:
        x = D.seeded_planes(2, H, W, 200 + layout)
    got = V.frames_to_yuv_host(x, H, W, layout, matrix, crange, bits=bits)
    pre, want = D.egress64(x, H, W, layout, matrix, crange, bits)
    assert got.shape == want.shape == (x.shape[0], V.frame_bytes(H, W, layout, bits)) and got.dtype == np.uint8
    got, want = got.view("<u2"), want.view("<u2")
    near_tie = np.abs(pre - np.floor(pre) - 0.5) < tie_guard(bits)
    share = float(near_tie.mean())
    print("egress bits %d layout %d matrix %d range %d: %.3f %% within %.2e of a tie, %d codes differ outside them"
          % (bits, layout, matrix, crange, 100 * share, tie_guard(bits), int((got != want)[~near_tie].sum())))
    assert share <= TIE_SHARE, share
    assert np.array_equal(got[~near_tie], want[~near_tie])
    n_y = H * W
    assert got[:, :n_y].min() == k["ylo"] and got[:, :n_y].max() == k["yhi"]          # luma reaches both of its bounds
    if bits == 16:
        assert share == 0.0          # whole numbers in exact arithmetic: nothing lies near a tie, so every code is compared
        n_c = D.dims(H, W, layout)[1] * D.dims(H, W, layout)[0]
        assert np.array_equal(got[:, :n_y], payload.view("<u2")[:, :n_y]) and np.array_equal(got[0], payload.view("<u2")[0]) and n_c > 0, \
            "in-gamut luma, and constant chroma, come back as themselves"
    else:
        assert got[:, n_y:].min() == k["clo"] and got[:, n_y:].max() == k["chi"]
