"""Letterboxed clips on the GPU, the two kernels: ssm_luma_counts_fwd against active_counts_host word for word, and
ssm_window_cut_fwd against cut_window_host byte for byte.  The streamed runs are in tests/test_hip_video_active_stream.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from video_clips import LAYOUTS, V, fbytes, random_payloads  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SIZES = ((1, 1), (3, 5), (17, 63), (33, 64), (64, 257))          # 33 rows: two bands; 257 columns: two column tiles; 64 and 257: both load paths
POISON = 0x5a5a5a5a


def counts(dev, h, w, bits, limit):
    """luma_counts of a device tensor into poisoned arrays -> (rows, cols) as numpy uint32."""
    n = dev.shape[0]
    rows = torch.full((n, h), POISON, dtype=torch.int32, device=DEV)
    cols = torch.full((n, w), POISON, dtype=torch.int32, device=DEV)
    V().luma_counts(dev, h, w, bits, limit, rows, cols)
    torch.cuda.synchronize()
    return rows.cpu().numpy().view(np.uint32), cols.cpu().numpy().view(np.uint32)


def check_counts(planes, h, w, bits, limit, slack=0):
    """Kernel == yardstick on numpy planes [N, plane bytes]; slack: bytes between the planes on the device (a stride above the plane)."""
    n, pb = planes.shape
    wide = torch.full((n, pb + slack), 0xff, dtype=torch.uint8, device=DEV)
    wide[:, :pb] = torch.from_numpy(planes).to(DEV)
    got = counts(wide[:, :pb], h, w, bits, limit)
    want = V().active_counts_host(planes, h, w, bits, limit)
    for g, x, name in zip(got, want, ("rows", "cols")):
        assert g.shape == x.shape and np.array_equal(g, x), (name, h, w, bits, limit, n, slack, g.tolist(), x.tolist())
    return got


@pytest.mark.parametrize("bits", [8, 10, 16])
@pytest.mark.parametrize("n", [1, 3])
def test_counts_equal_the_yardstick(bits, n):
    sb = 1 if bits == 8 else 2
    peak = (1 << bits) - 1
    for h, w in SIZES:
        planes = random_payloads(h, w, 2, sb, n, seed=bits)[:, :h * w * sb].copy()          # the luma plane of a 4:4:4 payload
        if bits == 10:
            planes.view("<u2")[...] &= peak
        for limit in (0, peak, peak // 2, None):
            check_counts(planes, h, w, bits, limit)
        check_counts(planes, h, w, bits, peak // 3, slack=2 * sb * 7)          # a frame stride larger than the frame, which leaves the alignment
        check_counts(planes, h, w, bits, peak // 3, slack=16)
        dark, bright = np.zeros_like(planes), np.full_like(planes, 0xff)
        if bits == 10:
            bright.view("<u2")[...] = peak
        rows, cols = check_counts(dark, h, w, bits, 0)
        assert not rows.any() and not cols.any(), "all dark: the poisoned arrays come back as zeros"
        rows, cols = check_counts(bright, h, w, bits, peak - 1)
        assert (rows == w).all() and (cols == h).all()
        rows, cols = check_counts(bright, h, w, bits, peak)
        assert not rows.any() and not cols.any(), "nothing is above the peak"


def test_counts_look_at_luma_alone_and_take_payload_rows():
    """Whole payloads as the loop holds them: rows of frame_bytes, the luma plane in front; two runs give equal words."""
    v = V()
    h, w = 34, 70
    for layout, bits in ((v.CENTRED, 8), (v.C422, 10)):
        sb = 1 if bits == 8 else 2
        clip = random_payloads(h, w, layout, sb, 3, seed=4)
        if bits == 10:
            clip.view("<u2")[...] &= 1023
        dev = torch.from_numpy(clip).to(DEV)
        got = counts(dev, h, w, bits, None)
        want = v.active_counts_host(clip, h, w, bits)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        again = counts(dev, h, w, bits, None)
        assert np.array_equal(got[0], again[0]) and np.array_equal(got[1], again[1])
        one = counts(dev[1:2], h, w, bits, None)
        assert np.array_equal(one[0], want[0][1:2]) and np.array_equal(one[1], want[1][1:2])


# ---- the cut -------------------------------------------------------------------------------------------------------------------------------
ALIGN = {0: (2, 2), 1: (2, 2), 2: (1, 1), 3: (1, 2)}          # layout -> (rows, columns)


def rects_of(h, w, layout):
    """A window at each corner, the whole frame and the smallest aligned window (inside, and on the far edges) of an h x w frame."""
    ay, ax = ALIGN[layout]
    my, mx = (h // 2) - (h // 2) % ay, (w // 2) - (w // 2) % ax
    return [(mx, my, 0, 0), (w - mx, my, mx, 0), (mx, h - my, 0, my), (w - mx, h - my, mx, my), (w, h, 0, 0), (ax, ay, mx, my),
            (w - (w - 1) // ax * ax, h - (h - 1) // ay * ay, (w - 1) // ax * ax, (h - 1) // ay * ay)]


@pytest.mark.parametrize("sb", [1, 2])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_cut_equals_the_yardstick(layout, sb):
    v = V()
    bits = 8 if sb == 1 else 16
    for h, w in ((17, 23), (32, 64), (35, 129)):          # odd sizes; rows of whole 16-byte pieces; rows of several pieces with a ragged end
        clip = random_payloads(h, w, layout, sb, 3, seed=6)
        dev = torch.from_numpy(clip).to(DEV)
        rects = rects_of(h, w, layout) + ([(32, 16, 16, 8), (48, 30, 16, 2)] if (h, w) == (32, 64) else [])
        for rect in rects:
            wb = v.frame_bytes(rect[1], rect[0], layout, bits)
            want = v.cut_window_host(clip, h, w, layout, bits, rect)
            got = v.window_cut(dev, h, w, layout, bits, rect)
            torch.cuda.synchronize()
            assert tuple(got.shape) == (3, wb) and np.array_equal(got.cpu().numpy(), want), (h, w, layout, sb, rect)
            # into wider rows, starting 2 bytes in: the destination's slack stays as it was
            wide = torch.full((3, wb + 10), 0xa5, dtype=torch.uint8, device=DEV)
            v.window_cut(dev, h, w, layout, bits, rect, out=wide[:, 2:2 + wb])
            torch.cuda.synchronize()
            host = wide.cpu().numpy()
            assert np.array_equal(host[:, 2:2 + wb], want), (h, w, layout, sb, rect)
            assert (host[:, :2] == 0xa5).all() and (host[:, 2 + wb:] == 0xa5).all(), "poisoned slack untouched"
        one = v.window_cut(dev[2:3], h, w, layout, bits, rects[3])
        torch.cuda.synchronize()
        assert np.array_equal(one.cpu().numpy(), v.cut_window_host(clip[2:3], h, w, layout, bits, rects[3]))


def test_cut_takes_frames_inside_wider_rows_and_refuses_a_misaligned_rectangle():
    v = V()
    h, w, layout, sb = 18, 22, v.CENTRED, 1
    clip = random_payloads(h, w, layout, sb, 2, seed=8)
    fb = fbytes(h, w, layout, sb)
    wide = torch.zeros(2, fb + 5, dtype=torch.uint8, device=DEV)
    wide[:, 3:3 + fb] = torch.from_numpy(clip).to(DEV)
    got = v.window_cut(wide[:, 3:3 + fb], h, w, layout, 8, (10, 8, 6, 4))
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), v.cut_window_host(clip, h, w, layout, 8, (10, 8, 6, 4)))
    with pytest.raises(RuntimeError, match="not aligned to \\(2,2\\)"):
        v.window_cut(wide[:, 3:3 + fb], h, w, layout, 8, (10, 8, 5, 4))
    with pytest.raises(RuntimeError, match="lies outside the 18x22 frame"):
        v.window_cut(wide[:, 3:3 + fb], h, w, layout, 8, (10, 8, 14, 4), out=torch.empty(2, 200, dtype=torch.uint8, device=DEV))
