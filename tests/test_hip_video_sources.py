"""The four readers in front of the streamed loop - FieldOrderSource, TelecineSource, RepeatSource, ActiveSource - on what they share
(ssm_amd.video.LookAheadSource): the end of a clip on and around a chunk boundary, probes against chunks, the sources stacked, and the
cost of a chunk.  40 x 56 frames; every expectation is the host definition's (detelecine_host, dedup_host, field_order_sums_host with
FieldVerdict.of_sums, active_area_host with ActiveArea.outside), never a source's own.

The empty stream, as the sources have always had it: TelecineSource and RepeatSource refuse it ("the Y4M stream holds no frame") when the
first frame is asked for; FieldOrderSource decides None over no inner frame and ActiveSource "no active row or column in the 0 probed
frames" (with a rectangle given: that rectangle), and both then hand out nothing."""
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import field_clips as FC  # noqa: E402
from video_clips import V  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
H, W = 40, 56
RATE = (30000, 1001)
RECT = (48, 32, 4, 4)          # (w, h, x, y) of the picture in the letterboxed clips
TAGS = ("420jpeg", "422p10")
CHUNKS = (1, 2, 5)
LENGTHS = (1, 2, 3, 5, 6, 7, 9, 10, 11)          # m c - 1, m c, m c + 1 for c = 1 (m = 2), 2 (m = 3) and 5 (m = 2); 1 and 2: below carry and probe


def fmt(tag):
    return V().EXTENDED_TAGS[tag]


def moving(n, tag, seed=3, bars=False, bright=()):
    """n frames of random legal codes, no two alike; bars: the picture inside RECT only, black around it, and in the frames of `bright`
    a white caption of two rows in the bottom bar."""
    v = V()
    layout, bits = fmt(tag)
    s = bits - 8
    rng = np.random.RandomState(seed)
    out = np.zeros((n, v.frame_bytes(H, W, layout, bits)), np.uint8)
    y, cu, cv = v.split_planes(out, H, W, layout, bits)
    y[...], cu[...], cv[...] = 16 << s, 128 << s, 128 << s
    rw, rh, x0, y0 = RECT if bars else (W, H, 0, 0)
    y[:, y0:y0 + rh, x0:x0 + rw] = rng.randint(64, 200, size=(n, rh, rw)) << s
    for i in bright:
        y[i, 37:39, 10:30] = 235 << s
    return out


def reader(payloads, tag, interlace="p"):
    v = V()
    buf = io.BytesIO()
    with v.Y4MWriter(buf, W, H, rate=RATE, aspect=(1, 1), chroma=tag, interlace=interlace, extended=True) as wr:
        for p in payloads:
            wr.write_frame(p)
    return v.Y4MReader(io.BytesIO(buf.getvalue()), extended=True, interlaced=True)


def drain(src, each=None):
    out, buf = [], np.empty(src.frame_bytes, np.uint8)
    while src.read_frame_into(buf):
        out.append(buf.copy())
        if each is not None:
            each()
    assert not src.read_frame_into(buf), "the end of the clip stays the end"
    return np.stack(out) if out else np.zeros((0, src.frame_bytes), np.uint8)


def same(got, want, case):
    assert got.keys() == want.keys()
    for key in want:
        if isinstance(want[key], np.ndarray):
            assert got[key].shape == want[key].shape and np.array_equal(got[key], want[key]), (case, key)
        else:
            assert got[key] == want[key], (case, key, got[key], want[key])


# ---- the four sources and their host definitions, as records that compare --------------------------------------------------------------
def telecined(n, tag):
    layout, bits = fmt(tag)
    return V().telecine_host(moving(20, tag), H, W, layout, bits, 0, 1)[:n]


def telecine_got(video, tag, wpc):
    src = V().TelecineSource(reader(video, tag, "t"), DEV, windows_per_chunk=wpc)
    frames = drain(src)
    return dict(frames=frames, read=src.frames_read, cadence=src.cadence, dropped=src.dropped, combed_first=src.combed_first)


def telecine_want(video, tag):
    layout, bits = fmt(tag)
    frames, cad = V().detelecine_host(video, H, W, layout, bits)
    return dict(frames=frames, read=len(frames), cadence=cad.log, dropped=cad.dropped, combed_first=cad.combed_first)


REPEATED = (0, 0, 1, 2, 2, 2, 3, 3, 3, 3, 4, 5, 5)          # runs of 1 and 2 repeats are repaired under dedup_max = 2, the run of 3 is a still


def repeated(n, tag):
    return moving(6, tag)[list(REPEATED[:n])]


def repeat_got(clip, tag, chunk):
    src = V().RepeatSource(reader(clip, tag), DEV, True, 2, frames_per_chunk=chunk)
    called, gaps = [], []
    src.on_gap = called.append
    frames = drain(src, lambda: gaps.append((src.gap, src.next_gap)))
    return dict(frames=frames, read=src.frames_read, repeats=src.repeats, gaps=gaps, on_gap=called)


def repeat_want(clip, tag):
    layout, bits = fmt(tag)
    acts, rep = V().dedup_host(clip, H, W, layout, bits, True, 2)
    kept = [n for n, a in acts if a is None]
    gap = [b - a for a, b in zip([0] + kept, kept)]
    return dict(frames=clip[kept], read=len(kept), repeats=rep.log, gaps=list(zip(gap, gap[1:] + [0])), on_gap=gap)


def field_got(clip, tag, probe, chunk):
    src = V().FieldOrderSource(reader(clip, tag), DEV, probe=probe, frames_per_chunk=chunk)
    verdict = src.decide()
    assert verdict == src.verdict
    frames = drain(src)
    return dict(frames=frames, read=src.frames_read, verdict=verdict, kinds=src.kinds, counts=src.counts, note=src.note, sums=np.asarray(src.sums))


def field_want(clip, tag, probe):
    v = V()
    p = clip[:probe]
    sums = v.field_order_sums_host(p[:-2], p[1:-1], p[2:], H, W, fmt(tag)[1]) if len(p) > 2 else np.zeros((0, 3), np.uint64)
    ref = v.FieldVerdict.of_sums(sums)
    return dict(frames=clip, read=len(clip), verdict=ref.verdict, kinds=ref.kinds, counts=ref.counts, note=ref.note, sums=sums)


def active_got(clip, tag, active, probe, chunk):
    src = V().ActiveSource(reader(clip, tag), DEV, active, probe, frames_per_chunk=chunk)
    area = src.decide()
    assert area == src.area
    frames = drain(src)
    return dict(frames=frames, read=src.frames_read, area=area, note=src.note, excess=src.excess)


def active_want(clip, tag, active, probe):
    v = V()
    layout, bits = fmt(tag)
    if active == "auto":
        rect, area = v.active_area_host(clip, H, W, layout, bits, probe=probe)
        note, first = area.note, min(probe, len(clip))
    else:
        rect, area, first = active, v.ActiveArea(H, W, layout), 0
        note = "the active area is %d:%d:%d:%d (W:H:X:Y), as given" % rect
    excess = []
    if rect is not None:
        for i in range(first, len(clip)):
            out = area.outside(*v.active_counts_host(clip[i], H, W, bits), rect)
            if out != (0, 0):
                excess.append((i,) + out)
    return dict(frames=clip, read=len(clip), area=rect, note=note, excess=excess)


# ---- 1. the end of the clip on and around a chunk boundary -----------------------------------------------------------------------------
def test_telecine_source_at_the_end_of_a_clip():
    """A chunk is 5 windows_per_chunk frames behind the first frame: 6, 11, 16 and 21 frames end on a boundary of both or of the smaller."""
    for tag, lengths in (("420jpeg", (6, 9, 10, 11, 16, 19, 20, 21)), ("422p10", (11,))):
        for n in lengths:
            video = telecined(n, tag)
            assert len(video) == n
            want = telecine_want(video, tag)
            assert want["dropped"] >= 1
            for wpc in (1, 2):
                same(telecine_got(video, tag, wpc), want, (tag, n, wpc))


def test_repeat_source_at_the_end_of_a_clip():
    """frames_per_chunk = 1 carries more frames (dedup_max + 1 = 3) than a chunk has; a one-frame clip is shorter than the carry."""
    for tag, lengths in (("420jpeg", LENGTHS + (13,)), ("422p10", (11,))):
        for n in lengths:
            clip = repeated(n, tag)
            want = repeat_want(clip, tag)
            if n == 13:
                assert [r[:3] for r in want["repeats"]] == [(1, 1, True), (4, 2, True), (7, 3, False), (12, 1, False)]
            for chunk in CHUNKS:
                same(repeat_got(clip, tag, chunk), want, (tag, n, chunk))


def test_field_order_source_at_the_end_of_a_clip():
    """The whole clip is probed; clips of 1 and 2 frames have no inner frame."""
    for tag, lengths in (("420jpeg", LENGTHS), ("422p10", (10,))):
        for n in lengths:
            clip = FC.payloads("bff", n, H, W, tag)
            want = field_want(clip, tag, 48)
            assert want["verdict"] == ("bff" if n > 2 else None) and len(want["kinds"]) == max(n - 2, 0)
            for chunk in CHUNKS:
                same(field_got(clip, tag, 48, chunk), want, (tag, n, chunk))


def test_active_source_at_the_end_of_a_clip():
    """The rectangle given - every frame is counted in chunks - and found over a probe of two frames with the chunks behind them; the
    last frame's caption lies outside."""
    for tag, lengths in (("420jpeg", LENGTHS), ("422p10", (10,))):
        for n in lengths:
            clip = moving(n, tag, bars=True, bright=(n - 1,) if n > 2 else ())
            for active in (RECT, "auto"):
                want = active_want(clip, tag, active, 2)
                assert want["area"] == RECT and [e[0] for e in want["excess"]] == ([n - 1] if n > 2 else [])
                for chunk in CHUNKS:
                    same(active_got(clip, tag, active, 2, chunk), want, (tag, n, active, chunk))


def test_the_empty_stream():
    v = V()
    tag = "420jpeg"
    none = np.zeros((0, v.frame_bytes(H, W, 0)), np.uint8)
    buf = np.empty(none.shape[1], np.uint8)
    for src in (v.TelecineSource(reader(none, tag), DEV), v.RepeatSource(reader(none, tag), DEV)):
        with pytest.raises(v.Y4MError, match="the Y4M stream holds no frame"):
            src.read_frame_into(buf)
    same(field_got(none, tag, 48, 2), field_want(none, tag, 48), "field order")
    got = field_got(none, tag, 48, 2)
    assert (got["verdict"], got["kinds"], got["counts"], got["read"]) == (None, "", (0, 0, 0, 0), 0)
    got = active_got(none, tag, "auto", 2, 2)
    assert (got["area"], got["note"], got["excess"], got["read"]) == (None, "no active row or column in the 0 probed frames", [], 0)
    same(active_got(none, tag, RECT, 2, 2), active_want(none, tag, RECT, 2), "active, as given")


# ---- 2. probe lengths against chunk sizes ------------------------------------------------------------------------------------------------
PROBES = (2, 3, 5, 7, 9)          # against chunks of 3 and clips of 7: below the chunk, the chunk, between the two, the clip, beyond it


def test_field_probes_against_chunks():
    clip = FC.payloads("tff", 7, H, W)
    for probe in PROBES:
        want = field_want(clip, "420jpeg", probe)
        assert len(want["kinds"]) == min(probe, 7) - 2 and (want["verdict"] == "tff" or probe == 2)
        for chunk in (3, 8):
            same(field_got(clip, "420jpeg", probe, chunk), want, (probe, chunk))


def test_active_probes_against_chunks():
    """Captions in frames 3 and 6: behind a probe of two frames and chunks of three, the first chunk and the last, partial one."""
    clip = moving(7, "420jpeg", bars=True, bright=(3, 6))
    for probe in PROBES:
        want = active_want(clip, "420jpeg", "auto", probe)
        if probe <= 3:
            assert want["area"] == RECT and [e[0] for e in want["excess"]] == [3, 6]
        else:
            assert want["area"] is not None and want["area"] != RECT, "a caption inside the probe widens the rectangle"
        for chunk in (3, 8):
            same(active_got(clip, "420jpeg", "auto", probe, chunk), want, (probe, chunk))


# ---- 3. stacking ---------------------------------------------------------------------------------------------------------------------------
def test_the_sources_stack():
    """Pulldown removal, then the active area, then the repeats, on a telecined letterboxed clip whose film repeats frame 5."""
    v = V()
    tag = "420jpeg"
    film = moving(11, tag, bars=True)[[0, 1, 2, 3, 4, 5, 5, 6, 7, 8, 9, 10]]
    video = v.telecine_host(film, H, W)
    back, _ = v.detelecine_host(video, H, W)
    acts, rep = v.dedup_host(back, H, W)
    assert rep.log == [(6, 1, True, 0, 0)]
    kept = [n for n, a in acts if a is None]
    base = reader(video, tag, "t")
    assert (base.interlace, base.field_order, base.field_bytes) == ("t", "tff", v.frame_bytes(H // 2, W, 0))
    tele = v.TelecineSource(base, DEV)
    active = v.ActiveSource(tele, DEV, RECT)
    top = v.RepeatSource(active, DEV)
    for layer in (tele, active, top):
        assert (layer.rate, layer.interlace, layer.bits, layer.frame_bytes, layer.field_order, layer.field_bytes) == \
            (v.detelecine_rate(RATE), "p", 8, base.frame_bytes, None, None)
        assert (layer.width, layer.height, layer.siting, layer.chroma, layer.aspect, layer.extended) == (W, H, 0, tag, (1, 1), True)
    got = drain(top)
    assert np.array_equal(got, back[kept]) and top.frames_read == len(kept) == len(back) - 1
    assert top.repeats == rep.log and tele.frames_read == active.frames_read == len(back)
    assert active.area == RECT and active.excess == [] and tele.dropped == len(video) - len(back)


# ---- 4. one stream, one wait ---------------------------------------------------------------------------------------------------------------
def test_a_chunk_is_measured_once(monkeypatch):
    """The cost of every source: one measuring step - one H2D, one kernel entry, its D2H, one event wait - per chunk, not per frame."""
    v = V()
    calls = []
    measure = v.LookAheadSource._measure
    monkeypatch.setattr(v.LookAheadSource, "_measure", lambda self, *a: calls.append(type(self).__name__) or measure(self, *a))
    tag, n, chunk = "420jpeg", 21, 5

    def steps(run):
        del calls[:]
        run()
        return len(calls)

    assert steps(lambda: telecine_got(telecined(n, tag), tag, 1)) == -(-(n - 1) // 5)          # behind the first frame
    assert steps(lambda: repeat_got(moving(n, tag), tag, chunk)) == -(-(n - 1) // chunk)
    boxed = moving(n, tag, bars=True)
    assert steps(lambda: active_got(boxed, tag, RECT, 48, chunk)) == -(-n // chunk)
    assert steps(lambda: active_got(boxed, tag, "auto", 7, chunk)) == -(-7 // chunk) + -(-(n - 7) // chunk)          # the probe, then the rest
    # the field probe: the chunks of the probed frames, but for a first one too short to close an inner frame
    assert steps(lambda: field_got(FC.payloads("tff", n, H, W), tag, 48, chunk)) == -(-n // chunk)
    assert steps(lambda: field_got(FC.payloads("tff", n, H, W), tag, 12, chunk)) == -(-12 // chunk)
    assert steps(lambda: field_got(FC.payloads("tff", n, H, W), tag, 48, 2)) == -(-n // 2) - 1
