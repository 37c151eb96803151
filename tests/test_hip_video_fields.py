"""Interlaced clips on the GPU, the two byte movers: ssm_fields_split_fwd and ssm_fields_weave_fwd against their numpy
yardsticks (ssm_amd.video.split_fields_host, weave_fields_host).  Bytes are moved and integers averaged: the results must be EQUAL.
What the shapes aim at: H = 2 (one row per field) and H = 4 in 4:2:0 (one-row chroma fields: both neighbours of a missing chroma row
clamp onto it), widths below a 16-byte piece, of exactly one, with a tail after whole pieces, odd ones (chroma of ceil(W / 2); rows that
start anywhere), every layout, bytes and words with every code (a word above the 10-bit peak passes through as it is), parity
alternating within a call, strides beyond a payload with the slack poisoned, and payloads that start 2 bytes off a 16-byte boundary, where
the sample-by-sample path runs in place of the 16-byte one.  Then every refusal, with its message, and nothing queued."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from video_clips import LAYOUTS, V, bits_of  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
FILL = 0xa7
HEIGHTS = (2, 4, 8, 12)
WIDTHS = (1, 2, 3, 16, 17, 33)
C420 = (0, 1)


def device_rows(rows, stride, shift):
    """numpy [N, L] uint8 -> a device view [N, L] of a poisoned flat buffer: row n starts `shift` + n * stride bytes into it.  Returns
    (the view, the flat buffer)."""
    n, length = rows.shape
    flat = torch.full((shift + n * stride + 32,), FILL, dtype=torch.uint8, device=DEV)
    view = flat[shift:shift + n * stride].view(n, stride)[:, :length]
    view.copy_(torch.from_numpy(np.ascontiguousarray(rows)).to(DEV))
    return view, flat


def poisoned_rows(n, length, stride, shift):
    flat = torch.full((shift + n * stride + 32,), FILL, dtype=torch.uint8, device=DEV)
    return flat[shift:shift + n * stride].view(n, stride)[:, :length], flat


def read_back(flat, n, length, stride, shift):
    """(the rows, whether every byte of the buffer outside them kept the poison), from one copy to the host."""
    host = flat.cpu().numpy()
    body = host[shift:shift + n * stride].reshape(n, stride)
    return body[:, :length], bool((host[:shift] == FILL).all() and (host[shift + n * stride:] == FILL).all() and (body[:, length:] == FILL).all())


def shapes(layout):
    for h in HEIGHTS:
        if h == 2 and layout in C420:
            continue
        for w in WIDTHS:
            yield h, w


def payloads(n, count, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(n, count)).astype(np.uint8)


@pytest.mark.parametrize("sb", [1, 2])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_split_equals_its_yardstick(layout, sb):
    v, bits = V(), bits_of(sb)
    for h, w in shapes(layout):
        fb = v.frame_bytes(h, w, layout, bits)
        for n in (1, 3):
            frames = payloads(n, fb, 31 * h + w + n)
            want = v.split_fields_host(frames, h, w, layout, bits)
            for shift in (0, 2):          # 2: no row of either operand starts on a 16-byte boundary
                src, _ = device_rows(frames, fb, shift)
                out, flat = poisoned_rows(2 * n, fb // 2, fb // 2, shift)
                assert v.fields_split(src, h, w, layout, bits, out=out).data_ptr() == out.data_ptr()
                got, clean = read_back(flat, 2 * n, fb // 2, fb // 2, shift)
                assert np.array_equal(got, want) and clean, (h, w, n, shift)


@pytest.mark.parametrize("sb", [1, 2])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_weave_equals_its_yardstick(layout, sb):
    v, bits = V(), bits_of(sb)
    for h, w in shapes(layout):
        fb = v.frame_bytes(h, w, layout, bits)
        hfb = fb // 2
        wide_f, wide_o = (hfb + 15) // 16 * 16 + 16, (fb + 15) // 16 * 16 + 32          # strides beyond a payload that keep rows on 16 bytes
        for n in (1, 3):
            kept, made = payloads(n, hfb, 17 * h + w + n), payloads(n, hfb, 19 * h + w + n)
            want = {(p0, fill): v.weave_fields_host(kept, None if fill else made, h, w, layout, bits, p0, fill) for p0 in (0, 1) for fill in (0, 1)}
            for shift, sf, so in ((0, wide_f, wide_o), (2, wide_f, wide_o), (0, hfb, fb)):
                dk, dm = device_rows(kept, sf, shift)[0], device_rows(made, sf, shift)[0]
                for (p0, fill), frames in want.items():
                    out, flat = poisoned_rows(n, fb, so, shift)
                    v.fields_weave(dk, None if fill else dm, h, w, layout, bits, p0, fill, out=out)
                    got, clean = read_back(flat, n, fb, so, shift)
                    assert np.array_equal(got, frames) and clean, (h, w, n, p0, fill, shift, sf)


@pytest.mark.parametrize("sb", [1, 2])
def test_a_frame_comes_back_from_its_own_fields_and_words_pass_through(sb):
    """weave(split(x)) = x on the device, more than one workgroup per frame (1024 pieces of 16 bytes each), 4:2:2 and 4:2:0; with words,
    every code above the 10-bit peak among them."""
    v, bits = V(), (8 if sb == 1 else 10)
    for layout, (h, w) in ((3, (36, 200)), (0, (40, 264))):
        frames = payloads(2, v.frame_bytes(h, w, layout, bits), h + w + sb)
        if sb == 2:
            assert (frames.view("<u2") > 1023).any()
        dev = torch.from_numpy(frames).to(DEV)
        fields = v.fields_split(dev, h, w, layout, bits)
        assert np.array_equal(fields.cpu().numpy(), v.split_fields_host(frames, h, w, layout, bits))
        # the parity of the kept rows alternates within a call: frame 0 keeps its top field (row 0), frame 1 its bottom field (row 3)
        back = v.fields_weave(fields[0::3], fields[1:3], h, w, layout, bits, v.TOP, 0)
        assert np.array_equal(back.cpu().numpy(), frames)
        back = v.fields_weave(fields[1:3], fields[0::3], h, w, layout, bits, v.BOTTOM, 0)
        assert np.array_equal(back.cpu().numpy(), frames)
        filled = v.fields_weave(fields[:3], None, h, w, layout, bits, v.BOTTOM, 1)
        assert np.array_equal(filled.cpu().numpy(), v.weave_fields_host(fields[:3].cpu().numpy(), None, h, w, layout, bits, v.BOTTOM, 1))


def test_weave_takes_strides_of_either_sign():
    v = V()
    h, w, layout = 8, 16, 2
    fb = v.frame_bytes(h, w, layout)
    kept, made = payloads(3, fb // 2, 5), payloads(3, fb // 2, 6)
    dk, dm = torch.from_numpy(kept).to(DEV), torch.from_numpy(made).to(DEV)
    out = torch.full((3, fb), FILL, dtype=torch.uint8, device=DEV)
    from ssm_amd import hipbind as hb
    hb.check(hb.load().ssm_fields_weave_fwd(dk.data_ptr() + 2 * (fb // 2), -(fb // 2), dm.data_ptr(), fb // 2, out.data_ptr() + 2 * fb, -fb, 3, h, w,
                                            layout, 1, 1, 0, hb.stream_ptr()))
    want = v.weave_fields_host(kept[::-1], made, h, w, layout, 8, 1, 0)[::-1]
    assert np.array_equal(out.cpu().numpy(), want)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_split_refusals_by_name_and_out_untouched():
    from ssm_amd import hipbind as hb
    n, h, w = 2, 8, 16
    fb = 8 * 16 * 3          # 4:4:4 bytes; every other layout and sample size of the calls below is smaller or refused before it matters
    frames = torch.zeros(2 * n * fb + 64, dtype=torch.uint8, device=DEV)
    out = torch.full((2 * n * fb + 64,), FILL, dtype=torch.uint8, device=DEV)

    def call(**kw):
        x = dict(frames=frames.data_ptr(), fields=out.data_ptr(), n=n, h=h, w=w, layout=2, bytes=1)
        x.update(kw)
        hb.check(hb.load().ssm_fields_split_fwd(x["frames"], x["fields"], x["n"], x["h"], x["w"], x["layout"], x["bytes"], hb.stream_ptr()))

    for bad, text in ((dict(frames=None), "fields_split: null pointer"), (dict(fields=None), "fields_split: null pointer"),
                      (dict(n=0), r"fields_split: N=0 outside 1\.\.65535"), (dict(n=65536), r"N=65536 outside 1\.\.65535"),
                      (dict(h=0), "fields_split: bad frame size 0x16"), (dict(w=0), "fields_split: bad frame size 8x0"),
                      (dict(layout=4), r"fields_split: layout 4 not in \{0, 1, 2, 3\}"), (dict(layout=-1), r"layout -1 not in"),
                      (dict(bytes=0), r"fields_split: sample_bytes 0 not in \{1, 2\}"), (dict(bytes=3), r"sample_bytes 3 not in \{1, 2\}"),
                      (dict(h=7), r"fields_split: an interlaced frame has an even number of rows \(H=7\)"),
                      (dict(h=6, layout=0), r"fields_split: an interlaced 4:2:0 frame has a multiple of 4 rows, two chroma fields of H/4 \(H=6\)"),
                      (dict(h=10, layout=1), r"multiple of 4 rows, two chroma fields of H/4 \(H=10\)"),
                      (dict(bytes=2, frames=frames.data_ptr() + 1), r"fields_split: a payload of 2-byte samples \(frames or fields\) is not 2-byte aligned"),
                      (dict(bytes=2, fields=out.data_ptr() + 1), r"2-byte samples \(frames or fields\) is not 2-byte aligned"),
                      (dict(fields=frames.data_ptr()), "fields_split: fields overlaps frames"),
                      (dict(fields=frames.data_ptr() + n * fb - 1), "fields overlaps frames"),
                      (dict(frames=out.data_ptr() + n * fb - 1), "fields overlaps frames")):
        with pytest.raises(RuntimeError, match=text):
            call(**bad)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == FILL).all(), "a refused call queues nothing"
    call(h=6, layout=3)          # 4:2:2 and 4:4:4 ask for an even H alone
    call(fields=frames.data_ptr() + n * fb)          # right behind the frames: no overlap
    call()
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert (host[:n * fb] == 0).all() and (host[n * fb:] == FILL).all()


def test_weave_refusals_by_name_and_out_untouched():
    from ssm_amd import hipbind as hb
    n, h, w = 3, 8, 16
    fb = 8 * 16 * 3
    half = fb // 2
    kept = torch.zeros(n * fb + 64, dtype=torch.uint8, device=DEV)
    made = torch.ones(n * fb + 64, dtype=torch.uint8, device=DEV)
    out = torch.full((n * 2 * fb + 64,), FILL, dtype=torch.uint8, device=DEV)

    def call(**kw):
        x = dict(kept=kept.data_ptr(), sk=half, made=made.data_ptr(), sm=half, out=out.data_ptr(), so=fb, n=n, h=h, w=w, layout=2, bytes=1,
                 parity0=0, fill=0)
        x.update(kw)
        hb.check(hb.load().ssm_fields_weave_fwd(x["kept"], x["sk"], x["made"], x["sm"], x["out"], x["so"], x["n"], x["h"], x["w"], x["layout"],
                                                x["bytes"], x["parity0"], x["fill"], hb.stream_ptr()))

    for bad, text in ((dict(kept=None), "fields_weave: null pointer"), (dict(out=None), "fields_weave: null pointer"),
                      (dict(made=None), "fields_weave: null pointer"),
                      (dict(n=0), r"fields_weave: N=0 outside 1\.\.65535"), (dict(n=65536), r"N=65536 outside 1\.\.65535"),
                      (dict(h=0), "fields_weave: bad frame size 0x16"), (dict(w=-1), "fields_weave: bad frame size 8x-1"),
                      (dict(layout=4), r"fields_weave: layout 4 not in \{0, 1, 2, 3\}"),
                      (dict(bytes=4), r"fields_weave: sample_bytes 4 not in \{1, 2\}"),
                      (dict(h=5), r"fields_weave: an interlaced frame has an even number of rows \(H=5\)"),
                      (dict(h=6, layout=0), r"fields_weave: an interlaced 4:2:0 frame has a multiple of 4 rows, two chroma fields of H/4 \(H=6\)"),
                      (dict(parity0=2), r"fields_weave: parity0 2 not in \{0, 1\}"), (dict(parity0=-1), r"parity0 -1 not in \{0, 1\}"),
                      (dict(fill=2), r"fields_weave: fill 2 not in \{0, 1\}"), (dict(fill=-1), r"fill -1 not in \{0, 1\}"),
                      (dict(bytes=2, kept=kept.data_ptr() + 1), r"fields_weave: a payload of 2-byte samples \(kept, made or frames\) is not 2-byte aligned"),
                      (dict(bytes=2, made=made.data_ptr() + 1), r"2-byte samples \(kept, made or frames\) is not 2-byte aligned"),
                      (dict(bytes=2, out=out.data_ptr() + 1), r"2-byte samples \(kept, made or frames\) is not 2-byte aligned"),
                      (dict(bytes=2, sk=2 * fb + 1, sm=2 * fb, so=2 * fb),
                       r"fields_weave: strides %d \(kept\), %d \(made\), %d \(frames\) of 2-byte samples must be even" % (2 * fb + 1, 2 * fb, 2 * fb)),
                      (dict(bytes=2, sk=2 * fb, sm=2 * fb, so=2 * fb + 1), r"of 2-byte samples must be even"),
                      (dict(sk=half - 1), r"fields_weave: strides %d \(kept\), %d \(made\) shorter than the field's %d bytes" % (half - 1, half, half)),
                      (dict(sm=-(half - 1)), r"strides %d \(kept\), -%d \(made\) shorter than the field's %d bytes" % (half, half - 1, half)),
                      (dict(sk=0), r"strides 0 \(kept\), %d \(made\) shorter than the field's" % half),
                      (dict(so=fb - 1), r"fields_weave: stride %d \(frames\) shorter than the frame's %d bytes" % (fb - 1, fb)),
                      (dict(so=0), r"stride 0 \(frames\) shorter than the frame's"),
                      (dict(out=kept.data_ptr()), "fields_weave: frames overlaps kept or made"),
                      (dict(out=made.data_ptr() + n * half - 1), "frames overlaps kept or made"),
                      (dict(kept=out.data_ptr() + n * fb - 1), "frames overlaps kept or made"),
                      (dict(kept=out.data_ptr() + half, n=1, fill=1, made=None), "frames overlaps kept or made")):
        with pytest.raises(RuntimeError, match=text):
            call(**bad)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == FILL).all(), "a refused call queues nothing"
    call(fill=1, made=None, sm=0)          # made is not read with fill = 1: it may be null
    call(fill=1, made=out.data_ptr(), sm=1)          # ... or anything else
    call(n=1, sk=0, sm=0, so=0, kept=out.data_ptr() + fb)          # N = 1: a stride names nothing; kept right behind the frame: no overlap
    call()
    torch.cuda.synchronize()
    host = out.cpu().numpy()[:n * fb].reshape(n, 3, h, w)
    assert (host[0, :, 0::2] == 0).all() and (host[0, :, 1::2] == 1).all() and (host[1, :, 1::2] == 0).all() and (host[1, :, 0::2] == 1).all()
    assert (out.cpu().numpy()[n * fb:] == FILL).all()
