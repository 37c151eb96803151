"""The letterboxed clip the active-area tests share (tests/test_video_active_cpu.py, test_hip_video_active_stream.py): the moving picture
clip of tests/video_clips.py at the size of the streamed tests, 64 x 96, inside a 96 x 112 frame with black bars on all four sides; the
bottom bar carries a "subtitle" - a block in Y, U and V that moves and changes its codes every frame.  The subtitle's luma stays at or
below the default limit (24 at 8 bits), so it is not active; `bright` makes it a caption that is.

A plain helper module (no fixtures, no collection hooks), imported as tests/video_clips.py is."""
import numpy as np

from video_clips import V, clip_payloads, deep_payloads

H, W = 64, 96                   # the picture: the frame of tests/test_hip_video_timeline.py
FH, FW = 96, 112                # the frame
RECT = (96, 64, 8, 16)          # (w, h, x, y) of the picture in the frame


def picture_clip(tag, n=6, seed=5):
    v = V()
    layout, bits = v.EXTENDED_TAGS[tag]
    return clip_payloads(n, H, W, layout, seed) if bits == 8 else deep_payloads(n, H, W, tag, seed)


def boxed(picture, tag, bright=()):
    """The picture payloads [n, frame_bytes(H, W)] inside the frame: black bars, the subtitle of frame i in the bottom bar.  bright: the
    frames whose subtitle is a white caption, far above any limit."""
    v = V()
    layout, bits = v.EXTENDED_TAGS[tag]
    s = bits - 8
    n = picture.shape[0]
    bars = np.zeros((n, v.frame_bytes(FH, FW, layout, bits)), np.uint8)
    y, cu, cv = v.split_planes(bars, FH, FW, layout, bits)
    y[...], cu[...], cv[...] = 16 << s, 128 << s, 128 << s
    for i in range(n):
        y[i, 84:90, 20 + 4 * i:60 + 4 * i] = (235 << s) if i in bright else ((17 + i % 8) << s)
        ry = slice(42, 45) if cu.shape[1] < FH else slice(84, 90)
        cu[i, ry, 10 + 2 * i:30 + 2 * i] = (100 + i) << s
        cv[i, ry, 10 + 2 * i:30 + 2 * i] = (150 - i) << s
    return v.paste_window_host(picture, bars, FH, FW, layout, bits, RECT, out=bars)


def letterboxed(tag, n=6, bright=()):
    """(the letterboxed clip [n, frame_bytes(FH, FW)], the picture clip [n, frame_bytes(H, W)]) in the format of a tag."""
    picture = picture_clip(tag, n)
    return boxed(picture, tag, bright), picture
