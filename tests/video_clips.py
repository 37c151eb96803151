"""The plain helpers the streamed-video GPU modules share (tests/test_hip_video.py, test_hip_video_timeline.py, test_hip_shutter.py,
test_hip_video_edges.py): a synthetic clip as Y4M payloads, as a file or a stream in memory, read back, and through VideoInterpolator.

A plain helper module (no fixtures, no collection hooks), imported as tests/train_refs.py is.
"""
import io

import numpy as np


def V():
    from ssm_amd import video
    return video


def clip_payloads(n, h, w, siting, seed=5):
    """A moving synthetic clip as Y4M payloads [n, frame_bytes] uint8 (through the yardstick's egress: legal limited-range codes)."""
    from ssm_amd.weights import synthetic_frames_u8, IMAGENET_MEAN, IMAGENET_STD
    v = V()
    rgb = synthetic_frames_u8(n, h, w, seed=seed).numpy().astype(np.float32) / np.float32(255.0)          # [n,3,h,w]
    x = (rgb - np.float32(IMAGENET_MEAN)[None, :, None, None]) / np.float32(IMAGENET_STD)[None, :, None, None]
    return v.frames_to_yuv_host(x, h, w, siting, v.default_matrix(h), v.LIMITED)


def write_clip(dst, payloads, h, w, chroma="420jpeg", rate=(30, 1), color_range=None):
    """The payloads as a Y4M stream into `dst`, a path or a binary file object."""
    v = V()
    with v.Y4MWriter(dst, w, h, rate=rate, aspect=(1, 1), chroma=chroma, color_range=color_range) as wr:
        for p in payloads:
            wr.write_frame(p)


def clip_file(payloads, h, w, chroma="420jpeg", rate=(30, 1)):
    """The clip as a stream in memory, rewound: what Y4MReader takes."""
    buf = io.BytesIO()
    write_clip(buf, payloads, h, w, chroma, rate)
    buf.seek(0)
    return buf


def read_clip(src):
    """(the reader, for its header; the frames [n, frame_bytes] uint8) of a path or a binary file object."""
    v = V()
    with v.Y4MReader(src) as r:
        frames, buf = [], np.empty(r.frame_bytes, np.uint8)
        while r.read_frame_into(buf):
            frames.append(buf.copy())
        return r, np.stack(frames)


def stream(m, cfg, payloads, h, w, chroma="420jpeg", rate=(30, 1), **kw):
    """The clip through VideoInterpolator(**kw): (header of the output, its frames).  The writer's rate is the command line's rule."""
    v = V()
    r = v.Y4MReader(clip_file(payloads, h, w, chroma, rate))
    sink = io.BytesIO()
    wr = v.Y4MWriter.like(sink, r, rate=kw.get("target_rate") or r.rate)
    count = v.VideoInterpolator(m, cfg, **kw).run(r, wr)
    assert count == wr.frames_written
    hdr, got = read_clip(io.BytesIO(sink.getvalue()))
    assert got.shape[0] == count
    return hdr, got
