"""The clip family of the field-order tests (tests/test_video_field_order_cpu.py, test_hip_video_field_order.py): a smooth texture that
moves in x and in y, sampled at field times.  Luma at field time t:

    rint(128 + 60 sin((x - 3 t) / 5 + 0.3 sin(y / 7)) + 40 sin((y - 1.5 t) / 9)),   clipped to 8 bits

Frame i of an interlaced clip weaves the times 2 i v and (2 i + 1) v by row parity (tff: the even rows are the earlier field); frame i of
the progressive clip is the texture at 2 i v; the still is the texture at 0.  No hard edge that moves by whole rows: such a shape biases
one parity.

A plain helper module (no fixtures, no collection hooks), imported as tests/video_clips.py is.
"""
import numpy as np

KINDS = ("tff", "bff", "progressive", "still")


def texture(h, w, t):
    """The luma plane [h, w] uint8 at field time t."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    v = 128 + 60 * np.sin((x - 3 * t) / 5 + 0.3 * np.sin(y / 7)) + 40 * np.sin((y - 1.5 * t) / 9)
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def luma_clip(kind, n, h, w, v=1.0):
    """n luma planes [n, h, w] uint8 of a clip of `kind` at speed v."""
    assert kind in KINDS
    out = np.empty((n, h, w), np.uint8)
    for i in range(n):
        if kind == "still":
            out[i] = texture(h, w, 0.0)
        elif kind == "progressive":
            out[i] = texture(h, w, 2 * i * v)
        else:
            early, late = texture(h, w, 2 * i * v), texture(h, w, (2 * i + 1) * v)
            top, bottom = (early, late) if kind == "tff" else (late, early)
            out[i, 0::2], out[i, 1::2] = top[0::2], bottom[1::2]
    return out


def payloads(kind, n, h, w, tag="420jpeg", v=1.0):
    """The clip as Y4M payloads [n, frame_bytes] uint8 in the format of a tag: the luma scaled to the depth, chroma at mid-grey."""
    from ssm_amd import video as V
    layout, bits = V.EXTENDED_TAGS[tag]
    luma = luma_clip(kind, n, h, w, v)
    out = np.empty((n, V.frame_bytes(h, w, layout, bits)), np.uint8)
    y, u, c = V.split_planes(out, h, w, layout, bits)
    y[...] = luma.astype(y.dtype) << (bits - 8)
    u[...] = 1 << (bits - 1)
    c[...] = 1 << (bits - 1)
    return out
