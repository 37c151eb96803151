"""Interlaced clips through the streamed loop: VideoInterpolator(deinterlace=) on the GPU.

A clip of 2n fields g_0 .. g_2n-1 is woven on the host into n interlaced frames, top field first (It) and bottom field first (Ib).  What
the tool must write is fixed by code this option does not touch: output f has g_f's bytes on the rows of g_f's parity, and for 0 < f <
2n - 1 the other rows are the odd output frames of the EXISTING VideoInterpolator(upsample_rate=2) run on the two progressive sub-clips
g_0, g_2, ... and g_1, g_3, ... (weave_fields_host puts the two together); outputs 0 and 2n - 1 are weave_fields_host(fill=1) of their own
field.  Everything is compared byte for byte."""
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from video_clips import V, clip_payloads, deep_payloads, frames_of, synthetic_model  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
RATE = (30, 1)


@pytest.fixture(scope="module")
def model():
    return synthetic_model(DEV)


def y4m(payloads, h, w, tag, interlace):
    v = V()
    buf = io.BytesIO()
    with v.Y4MWriter(buf, w, h, rate=RATE, aspect=(1, 1), chroma=tag, interlace=interlace, extended=True) as wr:
        for p in payloads:
            wr.write_frame(p)
    return io.BytesIO(buf.getvalue())


def interlaced(fields, fh, w, tag, order):
    """The 2n fields, in time order, as n woven frames of 2 fh x w: under tff the earlier field of a frame is its top field."""
    v = V()
    layout, bits = v.EXTENDED_TAGS[tag]
    early = v.TOP if order == "tff" else v.BOTTOM          # every frame keeps its earlier field on the rows of that parity
    return np.concatenate([v.weave_fields_host(fields[f:f + 1], fields[f + 1:f + 2], 2 * fh, w, layout, bits, early, 0) for f in range(0, len(fields), 2)])


def progressive(m, cfg, payloads, h, w, tag, **kw):
    """The existing tool at upsample_rate = 2 on a progressive clip: its output frames."""
    v = V()
    r = v.Y4MReader(y4m(payloads, h, w, tag, "p"), extended=True)
    sink = io.BytesIO()
    count = v.VideoInterpolator(m, cfg, upsample_rate=2, **kw).run(r, v.Y4MWriter.like(sink, r, rate=v.output_rate(r.rate, 2)))
    out = frames_of(sink.getvalue())
    assert out.shape[0] == count == 2 * len(payloads) - 1 and np.array_equal(out[0::2], payloads)
    return out


def expected(m, cfg, fields, fh, w, tag, order, **kw):
    """What deinterlacing the woven clip must write, from the existing tool's two runs and the two numpy yardsticks."""
    v = V()
    layout, bits = v.EXTENDED_TAGS[tag]
    n2 = len(fields)
    made = np.zeros_like(fields)
    made[1:n2 - 1:2] = progressive(m, cfg, fields[0::2], fh, w, tag, **kw)[1::2]          # between g_0 and g_2, ...: outputs 1, 3, ...
    if n2 > 2:
        made[2:n2 - 1:2] = progressive(m, cfg, fields[1::2], fh, w, tag, **kw)[1::2]      # between g_1 and g_3, ...: outputs 2, 4, ...
    p0 = v.field_of(0, order)[1]
    want = v.weave_fields_host(fields, made, 2 * fh, w, layout, bits, p0, 0)
    want[0] = v.weave_fields_host(fields[:1], None, 2 * fh, w, layout, bits, p0, 1)[0]
    want[-1] = v.weave_fields_host(fields[-1:], None, 2 * fh, w, layout, bits, v.field_of(n2 - 1, order)[1], 1)[0]
    return want


def deinterlace(m, cfg, frames, h, w, tag, interlace, mode="auto", **kw):
    """(header of the output, its frames) of VideoInterpolator(deinterlace=mode) on the clip with I`interlace` in its header."""
    v = V()
    r = v.Y4MReader(y4m(frames, h, w, tag, interlace), extended=True, interlaced=True)
    sink = io.BytesIO()
    wr = v.Y4MWriter.like(sink, r, rate=v.output_rate(r.rate, 2))
    count = v.VideoInterpolator(m, cfg, deinterlace=mode, **kw).run(r, wr)
    assert count == wr.frames_written == 2 * len(frames)
    data = sink.getvalue()
    hdr = v.Y4MReader(io.BytesIO(data), extended=True)
    return hdr, frames_of(data)


def check(m, cfg, fields, fh, w, tag, want_of=None, **kw):
    """Both field orders of one set of fields against the expected output; returns it per order."""
    v = V()
    layout, bits = v.EXTENDED_TAGS[tag]
    out = {}
    for order, interlace in (("tff", "t"), ("bff", "b")):
        frames = interlaced(fields, fh, w, tag, order)
        hdr, got = deinterlace(m, cfg, frames, 2 * fh, w, tag, interlace, **kw)
        assert got.shape[0] == len(fields)
        assert (hdr.interlace, hdr.rate, hdr.chroma, hdr.height, hdr.width, hdr.aspect) == ("p", (60, 1), tag, 2 * fh, w, (1, 1))
        back = v.split_fields_host(got, 2 * fh, w, layout, bits).reshape(len(fields), 2, -1)
        for f in range(len(fields)):
            assert np.array_equal(back[f, v.field_of(f, order)[1]], fields[f]), "output %d (%s): its own field's rows are not the input's bytes" % (f, order)
        want = expected(m, cfg, fields, fh, w, tag, order, **kw) if want_of is None else want_of[order]
        diff = [f for f in range(len(fields)) if not np.array_equal(got[f], want[f])]
        assert not diff, "%s: outputs %s differ from the fixed grid's fields / the line averages" % (order, diff)
        out[order] = want
    return out


@pytest.fixture(scope="module")
def clip420(model):
    """Ten 64 x 64 fields in 420jpeg and what the tool must write for them under both orders: computed once."""
    cfg, m = model
    fields = clip_payloads(10, 64, 64, 0)
    return fields, {order: expected(m, cfg, fields, 64, 64, "420jpeg", order) for order in ("tff", "bff")}


def test_it_and_ib_equal_the_fixed_grid_on_the_parity_streams(model, clip420):
    cfg, m = model
    fields, want = clip420
    check(m, cfg, fields, 64, 64, "420jpeg", want_of=want)


def test_422p10(model):
    cfg, m = model
    check(m, cfg, deep_payloads(10, 64, 64, "422p10"), 64, 64, "422p10")


def test_coarse_flow(model):
    cfg, m = model
    check(m, cfg, clip_payloads(10, 128, 128, 0), 128, 128, "420jpeg", flow_scale=2)


def test_tiled(model):
    cfg, m = model
    check(m, cfg, clip_payloads(10, 64, 192, 0), 64, 192, "420jpeg", tile=(64, 96), halo=32, blend=8)


def test_two_frames_per_pass_keep_count_order_and_fields(model, clip420):
    """pairs_per_batch = 2 over 4 new frames and then over the clip cut to 4 frames (3 new ones: the last pass is filled).  A two-pair pass
    runs its convolutions at batch 2: the bound is tests/test_hip_video.py's, for its reason - a code can flip at a tie, by one."""
    cfg, m = model
    v = V()
    fields, want = clip420
    for count in (10, 8):
        for order, interlace in (("tff", "t"), ("bff", "b")):
            frames = interlaced(fields[:count], 64, 64, "420jpeg", order)
            _, got = deinterlace(m, cfg, frames, 128, 64, "420jpeg", interlace, pairs_per_batch=2)
            back = v.split_fields_host(got, 128, 64, 0).reshape(count, 2, -1)
            for f in range(count):
                assert np.array_equal(back[f, v.field_of(f, order)[1]], fields[f])
            assert np.abs(got[:count - 1].astype(int) - want[order][:count - 1].astype(int)).max() <= 1
            last = v.weave_fields_host(fields[count - 1:count], None, 128, 64, 0, 8, v.field_of(count - 1, order)[1], 1)[0]
            assert np.array_equal(got[-1], last)


def test_one_frame_gives_two_filled_outputs(model):
    cfg, m = model
    v = V()
    fields = clip_payloads(2, 64, 64, 0)
    for order, interlace in (("tff", "t"), ("bff", "b")):
        frames = interlaced(fields, 64, 64, "420jpeg", order)
        assert frames.shape[0] == 1
        _, got = deinterlace(m, cfg, frames, 128, 64, "420jpeg", interlace)
        for f in (0, 1):
            want = v.weave_fields_host(fields[f:f + 1], None, 128, 64, 0, 8, v.field_of(f, order)[1], 1)[0]
            assert np.array_equal(got[f], want), (order, f)


def test_tff_overrides_a_progressive_header(model, clip420):
    cfg, m = model
    fields, want = clip420
    frames = interlaced(fields, 64, 64, "420jpeg", "tff")
    _, got = deinterlace(m, cfg, frames, 128, 64, "420jpeg", "p", mode="tff")
    assert np.array_equal(got, want["tff"])
    _, got = deinterlace(m, cfg, frames, 128, 64, "420jpeg", "t", mode="bff")          # the same bytes read bottom field first
    assert np.array_equal(got[0], V().weave_fields_host(V().split_fields_host(frames[:1], 128, 64, 0)[1:2], None, 128, 64, 0, 8, V().BOTTOM, 1)[0])
    with pytest.raises(ValueError, match='deinterlace="auto" takes the field order from the Y4M header, and this one says Ip'):
        deinterlace(m, cfg, frames, 128, 64, "420jpeg", "p", mode="auto")


def test_heights_without_fields_are_refused(model):
    cfg, m = model
    v = V()
    r = v.Y4MReader(y4m(clip_payloads(1, 66, 64, 0), 66, 64, "420jpeg", "p"))
    with pytest.raises(v.Y4MError, match="multiple of 4 rows"):
        v.VideoInterpolator(m, cfg, deinterlace="tff").run(r, v.Y4MWriter.like(io.BytesIO(), r))


def test_device_memory_is_flat_in_clip_length(model):
    cfg, m = model
    v = V()
    vi = v.VideoInterpolator(m, cfg, deinterlace="auto")
    peaks = []
    for n in (5, 5, 9):          # the first run also builds the plans
        frames = interlaced(clip_payloads(2 * n, 64, 64, 0), 64, 64, "420jpeg", "tff")
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(DEV)
        r = v.Y4MReader(y4m(frames, 128, 64, "420jpeg", "t"), interlaced=True)
        sink = open(os.devnull, "wb")
        assert vi.run(r, v.Y4MWriter.like(sink, r)) == 2 * n
        sink.close()
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated(DEV))
    print("peak device memory: 5 frames %d B, 9 frames %d B" % (peaks[1], peaks[2]))
    assert peaks[2] == peaks[1], peaks
