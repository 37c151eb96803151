"""The plain helpers the streamed-video GPU modules share (tests/test_hip_video.py, test_hip_video_timeline.py, test_hip_shutter.py,
test_hip_video_edges.py): a synthetic clip as Y4M payloads, as a file or a stream in memory, read back, and through VideoInterpolator.

Then what the modules of the sums over pairs of payloads share (test_hip_video_cuts.py, _score.py, _ssim.py, _mix.py, _holdout.py,
_holdout_ssim.py): the model with the synthetic weights, random payloads of a layout and sample width, and a clip in an extended format
through HoldOutScorer and through the existing tool.

A plain helper module (no fixtures, no collection hooks), imported as tests/train_refs.py is.
"""
import io

import numpy as np

CENTRED, COSITED, C444, C422 = 0, 1, 2, 3
LAYOUTS = (CENTRED, COSITED, C444, C422)


def V():
    from ssm_amd import video
    return video


def S():
    from ssm_amd import video_score
    return video_score


def synthetic_model(dev):
    """(cfg, FullModel with the synthetic weights on `dev`, in eval mode): what the modules' `model` fixtures return."""
    from models.superslomo_r import FullModel
    from ssm_amd.config import load_config, synthetic_weight_overrides
    from ssm_amd.weights import synthetic_state_dict
    cfg = load_config("superslomo_original.ini", synthetic_weight_overrides())
    m = FullModel(cfg)
    m.stage1_model.load_state_dict(synthetic_state_dict(1))
    m.stage2_model.load_state_dict(synthetic_state_dict(2))
    return cfg, m.to(dev).eval()


def bits_of(sb):
    return 8 if sb == 1 else 16


def fbytes(h, w, layout, sb):
    return V().frame_bytes(h, w, layout, bits_of(sb))


def random_payloads(h, w, layout, sb, n=3, seed=0):
    """n payloads of random bytes: every code of a byte, every one of the 65536 codes of a word."""
    rng = np.random.RandomState(1000 * h + 10 * w + layout + 7 * sb + seed)
    return rng.randint(0, 256, size=(n, fbytes(h, w, layout, sb))).astype(np.uint8)


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


# ---- clips in an extended format, scored -------------------------------------------------------------------------------------------------
def deep_payloads(n, h, w, tag, seed=5):
    """tests/test_hip_video_deep.py's deep_clip: a moving synthetic clip in the format of an extended tag."""
    from ssm_amd.weights import IMAGENET_MEAN, IMAGENET_STD, synthetic_frames_u8
    v = V()
    layout, bits = v.EXTENDED_TAGS[tag]
    rgb = synthetic_frames_u8(n, h, w, seed=seed).numpy().astype(np.float32) / np.float32(255.0)
    x = (rgb - np.float32(IMAGENET_MEAN)[None, :, None, None]) / np.float32(IMAGENET_STD)[None, :, None, None]
    return v.frames_to_yuv_host(x, h, w, layout, v.default_matrix(h), v.LIMITED, bits=bits)


def y4m(payloads, h, w, tag):
    v = V()
    buf = io.BytesIO()
    with v.Y4MWriter(buf, w, h, rate=(240, 1), aspect=(1, 1), chroma=tag, extended=True) as wr:
        for p in payloads:
            wr.write_frame(p)
    return io.BytesIO(buf.getvalue())


def frames_of(data):
    v = V()
    r = v.Y4MReader(io.BytesIO(data), extended=True)
    out, buf = [], np.empty(r.frame_bytes, np.uint8)
    while r.read_frame_into(buf):
        out.append(buf.copy())
    return np.stack(out) if out else np.zeros((0, r.frame_bytes), np.uint8)


def score(m, cfg, payloads, h, w, tag, hold, write=True, callbacks=None, **kw):
    """The clip through HoldOutScorer(**kw).run(reader, writer, **callbacks): (the result, the frames it wrote or None)."""
    v = V()
    r = v.Y4MReader(y4m(payloads, h, w, tag), extended=True)
    sink = io.BytesIO()
    wr = v.Y4MWriter.like(sink, r) if write else None
    res = S().HoldOutScorer(m, cfg, hold, **kw).run(r, wr, **(callbacks or {}))
    if not write:
        return res, None
    assert wr.frames_written == res.written
    return res, frames_of(sink.getvalue())


def reference(m, cfg, payloads, h, w, tag, hold, **kw):
    """The existing tool on the decimated clip: its output frames."""
    v = V()
    groups = (len(payloads) - 1) // hold
    r = v.Y4MReader(y4m(payloads[:groups * hold + 1:hold], h, w, tag), extended=True)
    sink = io.BytesIO()
    wr = v.Y4MWriter.like(sink, r)
    count = v.VideoInterpolator(m, cfg, upsample_rate=hold, **kw).run(r, wr)
    out = frames_of(sink.getvalue())
    assert out.shape[0] == count == groups * hold + 1
    return out
