"""3:2 pulldown removal through the streamed loop: TelecineSource on the GPU against detelecine_host, byte for byte and
window for window, and the tool end to end - a telecined clip through --detelecine gives the stream that the film clip it was made from
gives without it.  64 x 64 frames; the clips are made by telecine_host, which tests/test_video_detelecine_cpu.py holds to the film."""
import io
import logging
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from video_clips import V, clip_payloads, deep_payloads, frames_of, synthetic_model  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
H = W = 64
RATE = (30000, 1001)
TAGS = ("420jpeg", "422p10")


@pytest.fixture(scope="module")
def model():
    return synthetic_model(DEV)


def film_of(tag, n, seed=5):
    return clip_payloads(n, H, W, 0, seed=seed) if tag == "420jpeg" else deep_payloads(n, H, W, tag, seed=seed)


def y4m(payloads, tag, rate=RATE, interlace="p"):
    v = V()
    buf = io.BytesIO()
    with v.Y4MWriter(buf, W, H, rate=rate, aspect=(1, 1), chroma=tag, interlace=interlace, extended=True) as wr:
        for p in payloads:
            wr.write_frame(p)
    return io.BytesIO(buf.getvalue())


def source(video, tag, interlace="p", **kw):
    v = V()
    return v.TelecineSource(v.Y4MReader(y4m(video, tag, interlace=interlace), extended=True, interlaced=True), DEV, **kw)


def drain(src):
    out, buf = [], np.empty(src.frame_bytes, np.uint8)
    while src.read_frame_into(buf):
        out.append(buf.copy())
    assert not src.read_frame_into(buf), "the end of the clip stays the end"
    assert src.frames_read == len(out)
    return np.stack(out)


def clips(tag):
    """name -> telecined clip: both patterns at all five phases of nine film frames, a 26-frame clip whose cadence changes pattern and phase
    at frame 13, and a static clip."""
    v = V()
    layout, bits = v.EXTENDED_TAGS[tag]
    film = film_of(tag, 12)
    assert len({bytes(f) for f in film}) == len(film), "a moving clip: no two film frames alike"
    out = {"p%d q%d" % (pattern, phase): v.telecine_host(film[:9], H, W, layout, bits, pattern, phase) for pattern in (0, 1) for phase in range(5)}
    out["change at 13"] = np.concatenate([v.telecine_host(film, H, W, layout, bits, 0, 0)[:13],
                                          v.telecine_host(film_of(tag, 12, seed=6), H, W, layout, bits, 1, 2)[:13]])
    out["static"] = np.repeat(film[:1], 12, axis=0)
    return out


@pytest.mark.parametrize("tag", TAGS)
def test_source_equals_the_numpy_definition(tag):
    v = V()
    layout, bits = v.EXTENDED_TAGS[tag]
    for name, video in clips(tag).items():
        want, cadence = v.detelecine_host(video, H, W, layout, bits)
        got = {}
        for wpc in (1, 2):
            src = source(video, tag, windows_per_chunk=wpc)
            assert (src.interlace, src.rate, src.chroma, src.bits, src.height, src.width) == ("p", (24000, 1001), tag, bits, H, W)
            got[wpc] = drain(src)
            case = "%s, %d windows per chunk" % (name, wpc)
            assert got[wpc].shape == want.shape and np.array_equal(got[wpc], want), case
            assert src.cadence == cadence.log and src.dropped == cadence.dropped and src.combed_first == cadence.combed_first, case
            assert src.dropped == len(video) - len(want)
        assert np.array_equal(got[1], got[2]), name
        if name == "change at 13":
            # frames 13 .. 25 are frames 0 .. 12 of a pattern-1 clip at phase 2: q = (n - 11) % 5, phi = 1, h = 6; one frame dropped per window
            assert len(video) == 26 and [h for _, h, _, _ in cadence.log] == [0, 0, cadence.log[2][1], 6, 6] and len(want) == 21
        if name == "static":
            assert cadence.log == [(1, 0, 0, 0), (6, 0, 0, 0)]


def test_the_header_tag_is_not_needed():
    """It, Ib, Ip and I? over the same bytes give the same film: the field order falls out of the data."""
    v = V()
    video = v.telecine_host(film_of("420jpeg", 9), H, W, 0, 8, 1, 1)
    want, _ = v.detelecine_host(video, H, W)
    for interlace in ("t", "b", "p", "?"):
        assert np.array_equal(drain(source(video, "420jpeg", interlace)), want), interlace
    with pytest.raises(v.Y4MError, match="Im"):
        source(video, "420jpeg", "m")


def test_refusals_by_name():
    v = V()
    with pytest.raises(v.Y4MError, match="the clip has 5 frames, fewer than 6"):
        drain(source(film_of("420jpeg", 5), "420jpeg"))
    buf = io.BytesIO()
    with v.Y4MWriter(buf, W, 66, rate=RATE, chroma="420jpeg") as wr:
        wr.write_frame(np.zeros(v.frame_bytes(66, W, 0), np.uint8))
    with pytest.raises(v.Y4MError, match="a telecined frame in 4:2:0 has a multiple of 4 rows"):
        v.TelecineSource(v.Y4MReader(io.BytesIO(buf.getvalue())), DEV)


def test_memory_does_not_grow_with_the_clip():
    v = V()
    film = film_of("420jpeg", 9)
    peaks = []
    for cycles in (1, 1, 6):
        video = np.concatenate([v.telecine_host(film[:8], H, W, 0, 8, 0, 0)] * cycles)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(DEV)
        assert len(drain(source(video, "420jpeg"))) == 8 * cycles
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated(DEV))
    assert peaks[2] == peaks[1], peaks


def interpolate(m, cfg, reader, rate):
    v = V()
    sink = io.BytesIO()
    wr = v.Y4MWriter.like(sink, reader, rate=rate)
    count = v.VideoInterpolator(m, cfg, upsample_rate=2).run(reader, wr)
    wr.close()
    assert count == wr.frames_written
    return sink.getvalue()


@pytest.mark.parametrize("tag", TAGS)
def test_end_to_end_equals_the_run_on_the_film(model, tag):
    """Two whole cycles at phase 0: no frame is combed, and the telecined clip through TelecineSource is, to the interpolator, the film."""
    cfg, m = model
    v = V()
    layout, bits = v.EXTENDED_TAGS[tag]
    film = film_of(tag, 8)
    video = v.telecine_host(film, H, W, layout, bits, 0, 0)
    assert len(video) == 10
    src = source(video, tag)
    got = interpolate(m, cfg, src, v.output_rate(src.rate, 2))
    film_rate = v.detelecine_rate(RATE)
    want = interpolate(m, cfg, v.Y4MReader(y4m(film, tag, rate=film_rate), extended=True), v.output_rate(film_rate, 2))
    assert got == want, "header and frames, byte for byte"
    hdr = v.Y4MReader(io.BytesIO(got), extended=True)
    assert hdr.rate == (48000, 1001) and hdr.interlace == "p" and 5 * hdr.rate[0] * RATE[1] == 2 * 4 * RATE[0] * hdr.rate[1]
    frames = frames_of(got)
    assert len(frames) == 15 and np.array_equal(frames[0::2], film), "the film's frames pass through as their own bytes"
    # ten frames are frame 0, one window and a tail of four: frames 2 and 7 sit at q = 2
    assert len(src.cadence) == 1 and src.cadence[0][:3] == (1, 0, 0) and src.cadence[0][3] > 0 and src.dropped == 2 and not src.combed_first


def test_cli(model, tmp_path, caplog):
    import interpolate_video
    cfg, m = model
    v = V()
    film = film_of("420jpeg", 8)
    video = v.telecine_host(film, H, W, 0, 8, 1, 3)          # bottom field first, frame 0 at q = 3: written as it stands
    paths = {x: str(tmp_path / x) for x in ("in.y4m", "film.y4m", "out.y4m", "ref.y4m", "cfg.ini", "log.txt")}
    want_film, cadence = v.detelecine_host(video, H, W)
    for name, data in (("in.y4m", y4m(video, "420jpeg", interlace="t")), ("film.y4m", y4m(want_film, "420jpeg", rate=v.detelecine_rate(RATE)))):
        with open(paths[name], "wb") as f:
            f.write(data.getvalue())
    with open(paths["cfg.ini"], "w") as f:
        cfg.write(f)
    base = ["-c", paths["cfg.ini"], "--expt", "t", "--log", paths["log.txt"], "--fps", "60000:1001"]
    with caplog.at_level(logging.INFO):
        n = interpolate_video.main(base + ["--input", paths["in.y4m"], "--output", paths["out.y4m"], "--detelecine"], model=m)
    assert n == interpolate_video.main(base + ["--input", paths["film.y4m"], "--output", paths["ref.y4m"]], model=m)
    with open(paths["out.y4m"], "rb") as f, open(paths["ref.y4m"], "rb") as g:
        assert f.read() == g.read(), "24 -> 60 of the telecined clip is 24 -> 60 of its film"
    lines = [r.getMessage() for r in caplog.records if "detelecine" in r.getMessage()]
    assert any("30000:1001 frames/s in, film at 24000:1001" in ln for ln in lines)
    assert any("frame 0 sits at cadence position 3" in ln for ln in lines)
    assert sum("cadence h = 7 (bottom field first, phase 2)" in ln for ln in lines) == 1, lines
    assert any("%d windows, %d input frames dropped" % (len(cadence.log), cadence.dropped) in ln for ln in lines)
