"""ssm_field_diff_fwd on the GPU (pulldown removal): per pair of luma planes the sums of |a - b| over the rows of parity 0 and
of parity 1, against the numpy yardstick ssm_amd.video.field_diff_host.  Every sum is EQUAL: the kernel is integer arithmetic.  Every call
hands the entry a `sums` array full of ones in every bit, which it has to clear itself."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from video_clips import V, bits_of  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
POISON = 0xa7
GROUP = 1024          # pieces of 16 bytes to a workgroup: 256 lanes, 4 pieces each


def planes_ab(n, h, w, sb, seed=0):
    """Two sets of n random planes of h x w samples as bytes [n, h * w * sb]: every code of a byte, every one of the 65536 codes of a word."""
    rng = np.random.RandomState(7919 * h + 31 * w + 3 * sb + n + seed)
    return tuple(rng.randint(0, 256, size=(n, h * w * sb)).astype(np.uint8) for _ in range(2))


def on_device(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def diff(ta, tb, h, w, sb):
    """The binding on device tensors, `sums` filled with garbage before the call: [[top, bottom]] as Python integers."""
    out = torch.full((ta.shape[0], 2), -1, dtype=torch.int64, device=DEV)
    assert V().field_diff(ta, tb, h, w, bits_of(sb), out=out) is out
    return out.cpu().numpy().view(np.uint64).tolist()


def want(a, b, h, w, sb):
    return V().field_diff_host(a, b, h, w, bits_of(sb)).tolist()


@pytest.mark.parametrize("sb", (1, 2))
def test_sums_equal_the_yardstick(sb):
    """Rows shorter than a piece, a ragged piece after whole ones, whole pieces only; one row, odd numbers of rows; one pair and three.
    With three, planes 1 and 2 start wherever the plane's size puts them.  Behind every plane lie five samples, 0 in a and all ones in b,
    that a read past the plane would add."""
    for h in (1, 2, 3, 4, 9):
        for w in (1, 3, 16, 17, 33):
            for n in (1, 3):
                a, b = planes_ab(n, h, w, sb)
                pad = np.zeros((n, 5 * sb), np.uint8)
                ta, tb = on_device(np.hstack([a, pad])), on_device(np.hstack([b, pad + 255]))
                ref = want(a, b, h, w, sb)
                case = "h=%d w=%d n=%d" % (h, w, n)
                assert diff(ta, tb, h, w, sb) == ref == diff(tb, ta, h, w, sb), case
                assert diff(ta, ta, h, w, sb) == [[0, 0]] * n, case + ": a aliased to b"
                if h == 1:
                    assert all(row[1] == 0 for row in ref), "a single row has no bottom field"
                if n == 3:
                    assert diff(ta[1:2], tb[1:2], h, w, sb) == ref[1:2], case + ": N = 1 at plane 1's address"


@pytest.mark.parametrize("sb", (1, 2))
def test_whole_workgroup_loads_and_the_walk_over_rows(sb):
    """Planes on 16-byte boundaries with rows of whole pieces, more than one workgroup of them: the unguarded loads, and a last workgroup
    that goes piece by piece.  1008 and 1280 bytes to a row: 63 and 80 pieces, so a lane's next piece is 4 rows and 4 pieces, or 3 rows and
    16 pieces, further on - with and without a carry into the row."""
    for h, row in ((66, 1008), (48, 1280), (33, 4096)):
        w = row // sb
        assert row % 16 == 0 and h * (row // 16) > 2 * GROUP
        a, b = planes_ab(2, h, w, sb)
        ta, tb = on_device(a), on_device(b)
        assert (ta.data_ptr() | tb.data_ptr() | a.shape[1]) % 16 == 0
        ref = want(a, b, h, w, sb)
        assert len({s for r in ref for s in r}) == 4, "a sum booked under another parity or pair would show"
        assert diff(ta, tb, h, w, sb) == ref


@pytest.mark.parametrize("sb", (1, 2))
def test_payloads_off_a_16_byte_boundary(sb):
    """The same planes one sample past a 16-byte boundary, in a, in b and in both: nothing is loaded 16 bytes at a time where one of the
    two addresses does not allow it, and the poison around the planes stays out of the sums."""
    for h, w in ((4, 33), (9, 16), (3, 17), (40, 512 // sb)):
        a, b = planes_ab(2, h, w, sb, seed=1)
        size = a.size
        ref = want(a, b, h, w, sb)
        for off_a, off_b in ((sb, 0), (0, sb), (sb, sb)):
            bufs = []
            for x, off in ((a, off_a), (b, off_b)):
                buf = torch.full((size + 64,), POISON, dtype=torch.uint8, device=DEV)
                assert buf.data_ptr() % 16 == 0
                buf[16 + off:16 + off + size] = on_device(x.reshape(-1))
                bufs.append(buf[16 + off:16 + off + size].view(2, -1))
            assert bufs[0].data_ptr() % 16 == off_a and bufs[1].data_ptr() % 16 == off_b
            assert diff(bufs[0], bufs[1], h, w, sb) == ref, (h, w, off_a, off_b)


def raw(buf_a, first_a, stride_a, buf_b, first_b, stride_b, n, h, w, sb):
    """The entry point itself, for the strides a torch view cannot have: planes at buf + first + n * stride, in bytes."""
    from ssm_amd import hipbind as hb
    out = torch.full((n, 2), -1, dtype=torch.int64, device=DEV)
    hb.check(hb.load().ssm_field_diff_fwd(buf_a.data_ptr() + first_a, buf_b.data_ptr() + first_b, stride_a, stride_b, n, h, w, sb,
                                          out.data_ptr(), hb.stream_ptr()))
    return out.cpu().numpy().view(np.uint64).tolist()


def spread(planes, stride, first):
    """The planes `stride` bytes apart (either sign) in a poisoned device buffer, plane 0 at byte `first`."""
    n, size = planes.shape
    lo = min(0, (n - 1) * stride)
    host = np.full(first + abs((n - 1) * stride) + size + 32, POISON, np.uint8)
    for i in range(n):
        at = first - lo + i * stride
        host[at:at + size] = planes[i]
    return on_device(host), first - lo


@pytest.mark.parametrize("sb", (1, 2))
@pytest.mark.parametrize("h,w", ((9, 17), (4, 48)))
def test_strides_of_either_sign_and_one_plane_against_n(h, w, sb):
    n = 3
    a, b = planes_ab(n, h, w, sb, seed=2)
    size = a.shape[1]
    ref = want(a, b, h, w, sb)
    wide, wider = size + 6 * sb, 2 * size + 16          # beyond a plane: a ragged gap, and one that keeps the planes' alignment
    for sa, sb_ in ((wide, wider), (wider, -wide), (-wider, -wide), (-size, size)):
        (ba, fa), (bb, fb) = spread(a, sa, 16), spread(b, sb_, 32)
        assert raw(ba, fa, sa, bb, fb, sb_, n, h, w, sb) == ref, (sa, sb_)
    # stride 0: one plane of a against the three of b, and the other way round
    (ba, fa), (bb, fb) = spread(a[1:2], 0, 16), spread(b, wide, 16)
    assert raw(ba, fa, 0, bb, fb, wide, n, h, w, sb) == want(a[1:2], b, h, w, sb)
    (ba, fa), (bb, fb) = spread(a, -wide, 16), spread(b[2:3], 0, 48)
    assert raw(ba, fa, -wide, bb, fb, 0, n, h, w, sb) == want(a, b[2:3], h, w, sb)
    # and through the binding: an expanded row, and rows n + 1 against rows n of one buffer
    ta, tb = on_device(a), on_device(b)
    assert diff(ta[0:1].expand(n, size), tb, h, w, sb) == want(a[0:1], b, h, w, sb)
    assert diff(ta[1:], ta[:-1], h, w, sb) == want(a[1:], a[:-1], h, w, sb)


@pytest.mark.parametrize("sb", (1, 2))
def test_a_row_wider_than_a_workgroups_span(sb):
    h, w = 4, 16400 // sb
    assert w * sb // 16 == GROUP + 1, "a row is one piece more than a workgroup takes"
    a, b = planes_ab(1, h, w, sb)
    assert diff(on_device(a), on_device(b), h, w, sb) == want(a, b, h, w, sb)


@pytest.mark.parametrize("sb", (1, 2))
def test_many_rows(sb):
    h, w = 2050, 16
    a, b = planes_ab(2, h, w, sb)
    assert diff(on_device(a), on_device(b), h, w, sb) == want(a, b, h, w, sb)


def test_extreme_values():
    """Words 0 against 65535 at 64 x 4096: a parity's sum passes 2^32.  Bytes 0 against 255 at the same size."""
    h, w = 64, 4096
    for sb, peak in ((2, 65535), (1, 255)):
        a, b = np.zeros((2, h * w * sb), np.uint8), np.full((2, h * w * sb), 255, np.uint8)
        each = (h // 2) * w * peak
        assert (each > 1 << 32) == (sb == 2)
        assert diff(on_device(a), on_device(b), h, w, sb) == [[each, each]] * 2 == diff(on_device(b), on_device(a), h, w, sb)
