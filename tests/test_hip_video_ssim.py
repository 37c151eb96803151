"""SSIM of the hold-out score on the GPU: ssm_plane_ssim_fwd against its numpy yardstick (ssm_amd.video_score.plane_ssim_host).
The sums are fixed-point integers: every one must be EQUAL.  What the cases aim at: planes without a window, a tile that leaves its plane
or misses its last block column or row (single samples poked at either end of the covered area of every plane), trailing rows and columns
that must not count, planes at no particular alignment (the sample-by-sample loads), 32-bit block sums where 64 bits are needed, the
signed sum, strides of either sign and of 0, and the refusals."""
import os
import sys
import threading

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from video_clips import CENTRED, COSITED, C422, C444, LAYOUTS, S, bits_of, fbytes, random_payloads  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
ONE = 1 << 32
# A workgroup owns a tile of 31 x 15 windows of one plane, on 32 x 16 blocks of 4 x 4 samples (csrc/ssm_video.hip SSIM_TW, SSIM_TH).
TW, TH = 31, 15


def plane(wx, wy, extra=0):
    """(rows, cols) of a plane whose window grid is wx x wy, with `extra` trailing rows and columns."""
    return 4 * (wy + 1) + extra, 4 * (wx + 1) + extra


# (h, w), N = 3 payloads each.  2 x 2, 4 x 6: no window in any plane.  12 x 20: 2 x 4 windows in Y, the 6 x 10 chroma of 4:2:0 has none.
# 8 x 8: one window.  45 x 71, 46 x 70: planes that start anywhere, trailing rows and columns.  Then the Y plane's window grid one less
# than, equal to and one more than a tile in each direction (in 4:4:4 the chroma planes' too), and two tiles plus one window each way with
# trailing samples.
SIZES = ((2, 2), (4, 6), (12, 20), (8, 8), (45, 71), (46, 70),
         plane(TW - 1, TH - 1), plane(TW, TH), plane(TW + 1, TH + 1), plane(TW + 1, TH - 1, extra=1), plane(TW - 1, TH + 1, extra=3),
         plane(2 * TW + 1, 2 * TH + 1, extra=2))
assert plane(TW, TH) == (64, 128) and plane(2 * TW + 1, 2 * TH + 1, extra=2) == (130, 258)


def ssim(a, b, h, w, layout, sb, bits=None):
    """The device op on numpy payloads, `sums` filled with -1 before the call; the sums as Python integers [N][3]."""
    out = torch.full((a.shape[0], 3), -1, dtype=torch.int64, device=DEV)
    got = S().plane_ssim(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), h, w, layout, bits or bits_of(sb), out=out)
    assert got is out
    return out.cpu().tolist()


def want(a, b, h, w, layout, sb, bits=None):
    return S().plane_ssim_host(a, b, h, w, layout, bits or bits_of(sb)).tolist()


@pytest.mark.parametrize("sb", [1, 2])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("h,w", SIZES)
def test_kernel_equals_its_yardstick(h, w, layout, sb):
    a, b = random_payloads(h, w, layout, sb), random_payloads(h, w, layout, sb, seed=1)
    counts = S().plane_windows(h, w, layout)
    ref = want(a, b, h, w, layout, sb)
    assert all(row[p] == 0 for row in ref for p in range(3) if counts[p] == 0)
    assert ssim(a, b, h, w, layout, sb) == ref
    assert ssim(b, a, h, w, layout, sb) == ref
    assert ssim(a, a, h, w, layout, sb) == [[c * ONE for c in counts]] * 3, "a against a: every window is exactly 1; no window: 0, not the prefill"
    assert ssim(a[1:2], b[1:2], h, w, layout, sb) == ref[1:2], "N = 1, the payload at frame 1's address"
    if (h, w) in ((2, 2), (4, 6)):
        assert counts == (0, 0, 0) and ref == [[0, 0, 0]] * 3
    if (h, w) == (12, 20) and layout in (CENTRED, COSITED):
        assert counts == (8, 0, 0)


@pytest.mark.parametrize("bits", [10, 12])
def test_the_depth_enters_through_the_constants(bits):
    h, w, layout = 45, 71, C422
    a, b = random_payloads(h, w, layout, 2), random_payloads(h, w, layout, 2, seed=1)
    a.view("<u2")[:] &= (1 << bits) - 1
    b.view("<u2")[:] &= (1 << bits) - 1
    ref = want(a, b, h, w, layout, 2, bits)
    assert ssim(a, b, h, w, layout, 2, bits) == ref and ref != want(a, b, h, w, layout, 2, 16)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("h,w", [(45, 71), plane(TW + 1, TH + 1), plane(2 * TW + 1, 2 * TH + 1, extra=2)])
def test_extremes_and_the_signed_sum(h, w, layout):
    """0 against all-ones bytes: the largest block sums of either width (65535^2 * 16 per block passes 32 bits).  Random words are in the
    test above.  A checkerboard against its inverse: every window is close to -1."""
    from ssm_amd import video as V
    s = S()
    counts = s.plane_windows(h, w, layout)
    for sb in (1, 2):
        fb = fbytes(h, w, layout, sb)
        a, b = np.zeros((3, fb), np.uint8), np.full((3, fb), 255, np.uint8)
        ref = want(a, b, h, w, layout, sb)
        assert ssim(a, b, h, w, layout, sb) == ref == ssim(b, a, h, w, layout, sb)
        assert ssim(b, b, h, w, layout, sb) == [[c * ONE for c in counts]] * 3
        peak = 256 ** sb - 1
        ch, cw = V.chroma_dims(h, w, layout)
        boards = []
        for rows, cols in ((h, w), (ch, cw), (ch, cw)):
            yy, xx = np.mgrid[0:rows, 0:cols]
            boards.append((((yy + xx) & 1) * peak).ravel())
        board = np.concatenate(boards)
        dt = np.uint8 if sb == 1 else "<u2"
        a = board.astype(dt).view(np.uint8)[None]
        b = (peak - board).astype(dt).view(np.uint8)[None]
        got = ssim(a, b, h, w, layout, sb)
        assert got == want(a, b, h, w, layout, sb) and all(x < 0 for x, c in zip(got[0], counts) if c)


@pytest.mark.parametrize("sb", [1, 2])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("h,w", [(45, 71), plane(TW, TH), plane(TW + 1, TH + 1, extra=1), plane(2 * TW + 1, 2 * TH + 1, extra=2)])
def test_one_poked_sample_moves_its_own_plane_alone(h, w, layout, sb):
    """a = b except one sample of frame 1: the first or the last COVERED sample of Y, U or V moves that plane's sum of frame 1 alone (a
    tile that left its plane, or missed its last block row or column, would not); a sample of the trailing strip moves nothing."""
    from ssm_amd import video as V
    s = S()
    ch, cw = V.chroma_dims(h, w, layout)
    counts = s.plane_windows(h, w, layout)
    a = random_payloads(h, w, layout, sb)
    dt = np.uint8 if sb == 1 else "<u2"
    same = [[c * ONE for c in counts]] * 3
    starts = (0, h * w, h * w + ch * cw)
    for p, (rows, cols) in enumerate(((h, w), (ch, cw), (ch, cw))):
        if counts[p] == 0:
            continue
        last = (4 * (rows >> 2) - 1) * cols + 4 * (cols >> 2) - 1          # the last sample of the last block
        spots = [(0, True), (last, True)]
        if cols & 3:
            spots += [(cols - 1, False), (last + 1, False)]          # the trailing columns: end of row 0, and right after the last block
        if rows & 3:
            spots += [(rows * cols - 1, False), (4 * (rows >> 2) * cols, False)]          # the trailing rows: their last and first sample
        for at, covered in spots:
            b = a.copy()
            words = b.view(dt)
            words[1, starts[p] + at] ^= (0x55 if sb == 1 else 0xa5c3)
            got = ssim(a, b, h, w, layout, sb)
            if not covered:
                assert got == same, (p, at)
                continue
            assert got == want(a, b, h, w, layout, sb), (p, at)
            moved = [(n, q) for n in range(3) for q in range(3) if got[n][q] != same[n][q]]
            assert moved == [(1, p)], (p, at, moved)


def raw(a_ptr, b_ptr, sa, sb_, n, h, w, layout, sbytes, c1, c2, sums_ptr):
    from ssm_amd import hipbind as hb
    hb.check(hb.load().ssm_plane_ssim_fwd(a_ptr, b_ptr, sa, sb_, n, h, w, layout, sbytes, c1, c2, sums_ptr, hb.stream_ptr()))


@pytest.mark.parametrize("sb", [1, 2])
@pytest.mark.parametrize("h,w,layout", [(64, 96, CENTRED), (45, 71, CENTRED), (46, 70, C422), (68, 132, C444)])
def test_strides(h, w, layout, sb):
    s = S()
    bits = bits_of(sb)
    a = random_payloads(h, w, layout, sb, n=4, seed=2)
    fb = a.shape[1]
    buf = torch.from_numpy(a).to(DEV)
    out = torch.full((3, 3), -1, dtype=torch.int64, device=DEV)
    s.plane_ssim(buf[:-1], buf[1:], h, w, layout, bits, out=out)          # views of one buffer: frames n against n + 1
    assert out.cpu().tolist() == want(a[:-1], a[1:], h, w, layout, sb)
    one = buf[3:4].expand(3, fb)          # stride 0 on b: one frame against three
    assert one.stride(0) == 0
    got = s.plane_ssim(buf[:3], one, h, w, layout, bits).cpu().tolist()
    assert got == want(a[:3], a[3:4], h, w, layout, sb)
    assert s.plane_ssim(one, buf[:3], h, w, layout, bits).cpu().tolist() == got, "stride 0 on a"
    out = torch.full((4, 3), -1, dtype=torch.int64, device=DEV)          # a negative stride on a: frames 3, 2, 1 against 0, 1, 2
    c1, c2 = s.ssim_constants(bits)
    raw(buf.data_ptr() + 3 * fb, buf.data_ptr(), -fb, fb, 3, h, w, layout, sb, c1, c2, out.data_ptr())
    torch.cuda.synchronize()
    assert out.cpu().tolist() == want(a[3:0:-1], a[:3], h, w, layout, sb) + [[-1] * 3], "3 N words are written, no more"


def test_refusals_by_name_and_sums_untouched():
    h, w, n = 8, 12, 2          # 4:2:0: 144 bytes a frame, 288 as words
    a = torch.zeros(n, 400, dtype=torch.uint8, device=DEV)
    b = torch.ones(n, 400, dtype=torch.uint8, device=DEV)
    sums = torch.full((10,), -1, dtype=torch.int64, device=DEV)
    c1, c2 = S().ssim_constants(8)

    def call(**kw):
        x = dict(a=a.data_ptr(), b=b.data_ptr(), sa=400, sb=400, n=n, h=h, w=w, layout=CENTRED, bytes=1, c1=c1, c2=c2, sums=sums.data_ptr())
        x.update(kw)
        raw(x["a"], x["b"], x["sa"], x["sb"], x["n"], x["h"], x["w"], x["layout"], x["bytes"], x["c1"], x["c2"], x["sums"])

    for bad, text in ((dict(a=None), "plane_ssim: null pointer"), (dict(b=None), "plane_ssim: null pointer"), (dict(sums=None), "plane_ssim: null pointer"),
                      (dict(n=0), r"plane_ssim: N=0 outside 1\.\.65535"), (dict(n=65536), r"N=65536 outside 1\.\.65535"),
                      (dict(h=0), "plane_ssim: bad frame size 0x12"), (dict(w=-1), "bad frame size 8x-1"),
                      (dict(layout=4), r"plane_ssim: layout 4 not in \{0, 1, 2, 3\}"), (dict(layout=-1), "layout -1 not in"),
                      (dict(bytes=0), r"plane_ssim: sample_bytes 0 not in \{1, 2\}"), (dict(bytes=3), r"sample_bytes 3 not in \{1, 2\}"),
                      (dict(c1=0), r"plane_ssim: c1=0, c2=235963 outside 1\.\.2\^40"), (dict(c2=-5), r"c1=416, c2=-5 outside 1\.\.2\^40"),
                      (dict(c2=(1 << 40) + 1), r"c2=1099511627777 outside 1\.\.2\^40"),
                      (dict(sa=143), r"plane_ssim: strides 143 \(a\), 400 \(b\) neither 0 nor at least the frame's 144 bytes"),
                      (dict(sb=-143), r"strides 400 \(a\), -143 \(b\) neither 0 nor at least the frame's 144 bytes"),
                      (dict(bytes=2, sa=286), r"strides 286 \(a\), 400 \(b\) neither 0 nor at least the frame's 288 bytes"),
                      (dict(bytes=2, a=a.data_ptr() + 1), r"plane_ssim: a payload of 2-byte samples \(a or b\) is not 2-byte aligned"),
                      (dict(bytes=2, b=b.data_ptr() + 1), r"2-byte samples \(a or b\) is not 2-byte aligned"),
                      (dict(bytes=2, sa=399), r"plane_ssim: strides 399 \(a\), 400 \(b\) of 2-byte samples must be even"),
                      (dict(bytes=2, sb=-399), r"strides 400 \(a\), -399 \(b\) of 2-byte samples must be even"),
                      (dict(sums=sums.data_ptr() + 4), "plane_ssim: sums is not 8-byte aligned")):
        with pytest.raises(RuntimeError, match=text):
            call(**bad)
    torch.cuda.synchronize()
    assert sums.cpu().tolist() == [-1] * 10, "a refused call queues nothing: not even the clear"
    call()
    call(h=4, w=6, n=1, sa=0, sb=0, sums=sums.data_ptr() + 48)          # no window anywhere: the clear alone
    torch.cuda.synchronize()
    ref = S().plane_ssim_host(a.cpu().numpy()[:, :144], b.cpu().numpy()[:, :144], h, w, CENTRED, 8).tolist()
    assert sums.cpu().tolist() == ref[0] + ref[1] + [0, 0, 0, -1] and ref[0][0] > 0 and ref[0][1:] == [0, 0]


def test_two_host_threads_on_two_streams():
    """The entry point clears and sums on the caller's stream: two threads on two streams get the sums of the single-threaded call."""
    s = S()
    h, w, layout = plane(2 * TW + 1, 2 * TH + 1, extra=2) + (CENTRED,)
    cases = []
    for i, sb in enumerate((1, 2)):
        a, b = random_payloads(h, w, layout, sb, seed=10 + i), random_payloads(h, w, layout, sb, seed=20 + i)
        cases.append((torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), bits_of(sb), want(a, b, h, w, layout, sb)))
    outs = [[torch.full((3, 3), -1, dtype=torch.int64, device=DEV) for _ in range(4)] for _ in range(2)]
    streams = [torch.cuda.Stream(device=DEV) for _ in range(2)]
    errors, start = [], threading.Barrier(2)

    def worker(i):
        try:
            torch.cuda.set_device(DEV)
            ta, tb, bits, _ = cases[i]
            with torch.cuda.stream(streams[i]):
                start.wait()
                for rep in range(24):
                    s.plane_ssim(ta, tb, h, w, layout, bits, out=outs[i][rep % 4])
            streams[i].synchronize()
        except Exception as e:                              # noqa: BLE001 - reported by the asserting thread
            errors.append((i, repr(e)))

    torch.cuda.synchronize()
    threads = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for i in range(2):
        for o in outs[i]:
            assert o.cpu().tolist() == cases[i][3], "thread %d" % i
