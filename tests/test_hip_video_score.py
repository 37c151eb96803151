"""Hold-out scoring on the GPU: ssm_plane_sse_fwd against its numpy yardstick (ssm_amd.video_score.plane_sse_host).  The
kernel is integer arithmetic: every sum must be EQUAL.  What the cases aim at: a workgroup's span that crosses a plane boundary (single
samples poked at either end of every plane), planes that start at no particular alignment, a 32-bit sum where 64 bits are needed (the
16-bit extremes), strides of either sign and of 0, and the refusals."""
import os
import sys
import threading

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from video_clips import CENTRED, C422, C444, LAYOUTS, S, bits_of, fbytes, random_payloads  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
ONES = (1 << 64) - 1
# A workgroup sums a span of 16 KiB of one plane: 16384 samples of one byte, 8192 of two (csrc/ssm_video.hip SPAN_BYTES).
SPAN = 16384
# (h, w), N = 3 payloads each.  2 x 2: the chroma of 4:2:0 is 1 x 1.  4 x 6: less than one 16-byte piece per chroma plane.  45 x 71: odd frame
# bytes at 8 bits in 4:2:0 (4851) - frame 1 and the U plane (at byte 3195) start at odd bytes; at 16 bits the same counts in words.
# 46 x 70: even, no multiple of 16.  64 x 96: every plane on a 16-byte boundary, whole pieces, less than a span.  128 x 256 = 2 spans of
# bytes (4 of words) exactly, all planes aligned: the unguarded whole-span loads in every frame.  99 x 331 = 32769 = 2 spans + 1 sample
# (4 spans + 1 in words): frame 0's Y takes the whole-span loads and leaves one sample to a third workgroup, every other plane starts
# unaligned.  129 x 127 = 16383 = a span - 1 sample (two spans - 1 in words).
assert 99 * 331 == 2 * SPAN + 1 and 129 * 127 == SPAN - 1 and 128 * 256 == 2 * SPAN
SIZES = ((2, 2), (4, 6), (45, 71), (46, 70), (64, 96), (128, 256), (99, 331), (129, 127))


def sse(a, b, h, w, layout, sb):
    """The device op on numpy payloads, `sums` filled with ones before the call; the sums as Python integers [N][3]."""
    out = torch.full((a.shape[0], 3), -1, dtype=torch.int64, device=DEV)
    got = S().plane_sse(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), h, w, layout, bits_of(sb), out=out)
    assert got is out
    return out.cpu().numpy().view(np.uint64).tolist()


def want(a, b, h, w, layout, sb):
    return S().plane_sse_host(a, b, h, w, layout, bits_of(sb)).tolist()


@pytest.mark.parametrize("sb", [1, 2])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("h,w", SIZES)
def test_kernel_equals_its_yardstick(h, w, layout, sb):
    a, b = random_payloads(h, w, layout, sb), random_payloads(h, w, layout, sb, seed=1)
    ref = want(a, b, h, w, layout, sb)
    assert all(sum(row) > 0 for row in ref)
    assert sse(a, b, h, w, layout, sb) == ref
    assert sse(b, a, h, w, layout, sb) == ref
    assert sse(a, a, h, w, layout, sb) == [[0, 0, 0]] * 3
    assert sse(a[1:2], b[1:2], h, w, layout, sb) == ref[1:2], "N = 1, the payload at frame 1's address"


@pytest.mark.parametrize("sb", [1, 2])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("h,w", [(2, 2), (45, 71), (64, 96), (99, 331), (129, 127)])
def test_one_poked_sample_lands_in_its_own_plane(h, w, layout, sb):
    """a = b except one sample, the first or the last of Y, U or V of frame 1: that plane's sum is d^2, the other eight sums of the call
    are 0 - a span that crossed a plane boundary would book it with the neighbour."""
    s = S()
    y, u, v = s.plane_samples(h, w, layout)
    a = random_payloads(h, w, layout, sb)
    dt = np.uint8 if sb == 1 else "<u2"
    for p, at in ((0, 0), (0, y - 1), (1, y), (1, y + u - 1), (2, y + u), (2, y + u + v - 1)):
        b = a.copy()
        words = b.view(dt)
        old = int(words[1, at])
        new = old ^ (0x55 if sb == 1 else 0xa5c3)
        words[1, at] = new
        expect = [[0, 0, 0] for _ in range(3)]
        expect[1][p] = (new - old) ** 2
        assert sse(a, b, h, w, layout, sb) == expect, (p, at)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("h,w", [(64, 96), (99, 331), (45, 71)])
def test_extremes(h, w, layout):
    """0 against 255: 65025 per sample.  0 against 65535: 2^32 - 131071 per sample, which two samples carry past 32 bits."""
    samples = S().plane_samples(h, w, layout)
    for sb, d2 in ((1, 65025), (2, (1 << 32) - 131071)):
        fb = fbytes(h, w, layout, sb)
        a, b = np.zeros((3, fb), np.uint8), np.full((3, fb), 255, np.uint8)
        assert d2 == (256 ** sb - 1) ** 2
        expect = [[d2 * n for n in samples]] * 3
        assert sse(a, b, h, w, layout, sb) == expect == sse(b, a, h, w, layout, sb)
        assert expect == want(a, b, h, w, layout, sb)


def raw(a_ptr, b_ptr, sa, sb_, n, h, w, layout, sbytes, sums_ptr):
    from ssm_amd import hipbind as hb
    hb.check(hb.load().ssm_plane_sse_fwd(a_ptr, b_ptr, sa, sb_, n, h, w, layout, sbytes, sums_ptr, hb.stream_ptr()))


@pytest.mark.parametrize("sb", [1, 2])
@pytest.mark.parametrize("h,w,layout", [(64, 96, CENTRED), (45, 71, CENTRED), (46, 70, C422), (99, 331, C444)])
def test_strides(h, w, layout, sb):
    s = S()
    bits = bits_of(sb)
    a = random_payloads(h, w, layout, sb, n=4, seed=2)
    fb = a.shape[1]
    buf = torch.from_numpy(a).to(DEV)
    assert s.plane_sse(buf, buf, h, w, layout, bits).cpu().tolist() == [[0, 0, 0]] * 4, "a is b"
    out = torch.full((3, 3), -1, dtype=torch.int64, device=DEV)
    s.plane_sse(buf[:-1], buf[1:], h, w, layout, bits, out=out)          # views of one buffer: frames n against n + 1
    assert out.cpu().numpy().view(np.uint64).tolist() == want(a[:-1], a[1:], h, w, layout, sb)
    wide = buf[::2]
    assert wide.stride(0) == 2 * fb
    assert s.plane_sse(wide, buf[1::2], h, w, layout, bits).cpu().numpy().view(np.uint64).tolist() == want(a[::2], a[1::2], h, w, layout, sb)
    one = buf[3:4].expand(3, fb)          # stride 0 on b: one frame against three
    assert one.stride(0) == 0
    got = s.plane_sse(buf[:3], one, h, w, layout, bits).cpu().numpy().view(np.uint64).tolist()
    assert got == want(a[:3], a[3:4], h, w, layout, sb) and got == [want(a[i:i + 1], a[3:4], h, w, layout, sb)[0] for i in range(3)]
    assert s.plane_sse(one, buf[:3], h, w, layout, bits).cpu().numpy().view(np.uint64).tolist() == got, "stride 0 on a"
    out = torch.full((4, 3), -1, dtype=torch.int64, device=DEV)          # a negative stride on a: frames 3, 2, 1 against 0, 1, 2
    raw(buf.data_ptr() + 3 * fb, buf.data_ptr(), -fb, fb, 3, h, w, layout, sb, out.data_ptr())
    torch.cuda.synchronize()
    assert out.cpu().numpy().view(np.uint64).tolist() == want(a[3:0:-1], a[:3], h, w, layout, sb) + [[ONES] * 3], "3 N words are written, no more"


def test_refusals_by_name_and_sums_untouched():
    h, w, n = 8, 12, 2          # 4:2:0: 144 bytes a frame, 288 as words
    a = torch.zeros(n, 400, dtype=torch.uint8, device=DEV)
    b = torch.ones(n, 400, dtype=torch.uint8, device=DEV)
    sums = torch.full((10,), -1, dtype=torch.int64, device=DEV)

    def call(**kw):
        x = dict(a=a.data_ptr(), b=b.data_ptr(), sa=400, sb=400, n=n, h=h, w=w, layout=CENTRED, bytes=1, sums=sums.data_ptr())
        x.update(kw)
        raw(x["a"], x["b"], x["sa"], x["sb"], x["n"], x["h"], x["w"], x["layout"], x["bytes"], x["sums"])

    for bad, text in ((dict(a=None), "plane_sse: null pointer"), (dict(b=None), "plane_sse: null pointer"), (dict(sums=None), "plane_sse: null pointer"),
                      (dict(n=0), r"N=0 outside 1\.\.65535"), (dict(n=65536), r"N=65536 outside 1\.\.65535"),
                      (dict(h=0), "bad frame size 0x12"), (dict(w=-1), "bad frame size 8x-1"),
                      (dict(layout=4), r"layout 4 not in \{0, 1, 2, 3\}"), (dict(layout=-1), "layout -1 not in"),
                      (dict(bytes=0), r"sample_bytes 0 not in \{1, 2\}"), (dict(bytes=3), r"sample_bytes 3 not in \{1, 2\}"),
                      (dict(sa=143), r"strides 143 \(a\), 400 \(b\) neither 0 nor at least the frame's 144 bytes"),
                      (dict(sb=-143), r"strides 400 \(a\), -143 \(b\) neither 0 nor at least the frame's 144 bytes"),
                      (dict(bytes=2, sa=286), r"strides 286 \(a\), 400 \(b\) neither 0 nor at least the frame's 288 bytes"),
                      (dict(bytes=2, a=a.data_ptr() + 1), r"2-byte samples \(a or b\) is not 2-byte aligned"),
                      (dict(bytes=2, b=b.data_ptr() + 1), r"2-byte samples \(a or b\) is not 2-byte aligned"),
                      (dict(bytes=2, sa=399), r"strides 399 \(a\), 400 \(b\) of 2-byte samples must be even"),
                      (dict(bytes=2, sb=-399), r"strides 400 \(a\), -399 \(b\) of 2-byte samples must be even"),
                      (dict(sums=sums.data_ptr() + 4), "sums is not 8-byte aligned")):
        with pytest.raises(RuntimeError, match=text):
            call(**bad)
    torch.cuda.synchronize()
    assert sums.cpu().numpy().view(np.uint64).tolist() == [ONES] * 10, "a refused call queues nothing: not even the clear"
    call()
    call(bytes=2, n=1, sa=0, sb=0, sums=sums.data_ptr() + 48)
    torch.cuda.synchronize()
    y, c = h * w, h * w // 4          # 8-bit: 0 against 1; words: 0 against 0x0101 = 257
    assert sums.cpu().numpy().view(np.uint64).tolist() == [y, c, c, y, c, c, 66049 * y, 66049 * c, 66049 * c, ONES]


def test_two_host_threads_on_two_streams():
    """The entry point clears and sums on the caller's stream: two threads on two streams, as tests/test_hip_threads.py drives the
    convolutions, get the sums of the single-threaded call."""
    s = S()
    h, w, layout = 99, 331, CENTRED
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
                    s.plane_sse(ta, tb, h, w, layout, bits, out=outs[i][rep % 4])
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
            assert o.cpu().numpy().view(np.uint64).tolist() == cases[i][3], "thread %d" % i
