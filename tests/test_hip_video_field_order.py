"""ssm_field_order_sums_fwd, FieldOrderSource and VideoInterpolator(field_probe=) on the GPU (the field order from the data).

The kernel: per frame the comb sums (A0, A1, D) of its luma plane against the frame before and the frame after, against the numpy
yardstick ssm_amd.video.field_order_sums_host.  Every sum is EQUAL: the kernel is integer arithmetic.  Every call hands the entry a `sums`
array full of ones in every bit, which it has to clear itself.

The stream: texture clips of tests/field_clips.py under an Ip header.  What a probed run must write is fixed by code the option does not
touch: the run with the order given by name.  Everything is compared byte for byte."""
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import field_clips as FC  # noqa: E402
from video_clips import V, bits_of, frames_of, synthetic_model  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
POISON = 0xa7
GROUP, BAND = 256, 8          # units to a workgroup (a unit: one 16-byte piece of the rows over a band of 8 rows)


def planes3(n, h, w, sb, seed=0):
    """Three sets of n random planes of h x w samples as bytes [n, h * w * sb]: every code of a byte, every one of the 65536 of a word."""
    rng = np.random.RandomState(7919 * h + 31 * w + 3 * sb + n + seed)
    return tuple(rng.randint(0, 256, size=(n, h * w * sb)).astype(np.uint8) for _ in range(3))


def on_device(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def sums(tp, tc, tn, h, w, sb):
    """The binding on device tensors, `sums` filled with garbage before the call: [[A0, A1, D]] as Python integers."""
    out = torch.full((tc.shape[0], 3), -1, dtype=torch.int64, device=DEV)
    assert V().field_order_sums(tp, tc, tn, h, w, bits_of(sb), out=out) is out
    return out.cpu().numpy().view(np.uint64).tolist()


def want(p, c, n, h, w, sb):
    return V().field_order_sums_host(p, c, n, h, w, bits_of(sb)).tolist()


@pytest.mark.parametrize("sb", (1, 2))
def test_sums_equal_the_yardstick(sb):
    """No inner row, one, two, many with a last band that is not whole; rows shorter than a piece, a ragged piece after whole ones, whole
    pieces only, row pitches that are no multiple of 16; one frame, three, seven.  Planes 1 .. start wherever the plane's size puts them.
    Behind every plane lie five samples, 0 in c and all ones in p and n, that a read past the plane would add."""
    for h in (1, 2, 3, 4, 37):
        for w in (1, 15, 16, 17, 53):
            for n in (1, 3, 7):
                p, c, nx = planes3(n, h, w, sb)
                pad = np.zeros((n, 5 * sb), np.uint8)
                tp, tc, tn = on_device(np.hstack([p, pad + 255])), on_device(np.hstack([c, pad])), on_device(np.hstack([nx, pad + 255]))
                ref = want(p, c, nx, h, w, sb)
                case = "h=%d w=%d n=%d" % (h, w, n)
                assert sums(tp, tc, tn, h, w, sb) == ref, case
                assert sums(tn, tc, tp, h, w, sb) == [[a1, a0, d] for a0, a1, d in ref], case + ": p and n exchanged exchange A0 and A1"
                assert sums(tc, tc, tc, h, w, sb) == want(c, c, c, h, w, sb), case + ": p = c = n aliased"
                if h < 3:
                    assert ref == [[0, 0, 0]] * n
                if n == 3:
                    assert sums(tp[1:2], tc[1:2], tn[1:2], h, w, sb) == ref[1:2], case + ": N = 1 at plane 1's address"


@pytest.mark.parametrize("sb", (1, 2))
def test_whole_bands_and_more_than_one_workgroup_along_both_axes(sb):
    """Planes on 16-byte boundaries with rows of whole pieces: the unguarded loads of the whole bands, the guarded walk of a last band that
    is not whole, more than one workgroup of units and more than one frame."""
    for h, row in ((67, 1008), (48, 1280), (35, 4096)):
        w = row // sb
        units = (row // 16) * -(-(h - 2) // BAND)
        assert row % 16 == 0 and units > GROUP and (h - 2) % BAND != 0
        p, c, nx = planes3(2, h, w, sb)
        tp, tc, tn = on_device(p), on_device(c), on_device(nx)
        assert (tp.data_ptr() | tc.data_ptr() | tn.data_ptr() | p.shape[1]) % 16 == 0
        ref = want(p, c, nx, h, w, sb)
        assert len({s for r in ref for s in r}) == 6, "a sum booked under another word or frame would show"
        assert sums(tp, tc, tn, h, w, sb) == ref
    h, w = 2 + 2 * BAND, 8 * GROUP          # every band whole
    p, c, nx = planes3(3, h, w, sb, seed=4)
    assert sums(on_device(p), on_device(c), on_device(nx), h, w, sb) == want(p, c, nx, h, w, sb)


@pytest.mark.parametrize("sb", (1, 2))
def test_payloads_off_a_16_byte_boundary(sb):
    """The same planes one sample past a 16-byte boundary, in each operand and in all: nothing is loaded 16 bytes at a time where the
    address does not allow it, and the poison around the planes stays out of the sums."""
    for h, w in ((4, 33), (11, 16), (3, 17), (37, 512 // sb)):
        p, c, nx = planes3(2, h, w, sb, seed=1)
        size = p.size
        ref = want(p, c, nx, h, w, sb)
        for offs in ((sb, 0, 0), (0, sb, 0), (0, 0, sb), (sb, sb, sb)):
            bufs = []
            for x, off in zip((p, c, nx), offs):
                buf = torch.full((size + 64,), POISON, dtype=torch.uint8, device=DEV)
                assert buf.data_ptr() % 16 == 0
                buf[16 + off:16 + off + size] = on_device(x.reshape(-1))
                bufs.append(buf[16 + off:16 + off + size].view(2, -1))
            assert [b.data_ptr() % 16 for b in bufs] == list(offs)
            assert sums(*bufs, h, w, sb) == ref, (h, w, offs)


def raw(bufs, firsts, strides, n, h, w, sb, guard=0):
    """The entry point itself, for the strides a torch view cannot have: planes at buf + first + i * stride, in bytes.  guard: poisoned
    words on either side of `sums`, returned with it."""
    from ssm_amd import hipbind as hb
    out = torch.full((3 * n + 2 * guard,), -1, dtype=torch.int64, device=DEV)
    hb.check(hb.load().ssm_field_order_sums_fwd(*(b.data_ptr() + f for b, f in zip(bufs, firsts)), *strides, n, h, w, sb,
                                                out.data_ptr() + 8 * guard, hb.stream_ptr()))
    got = out.cpu().numpy().view(np.uint64)
    if guard:
        return got[guard:-guard].reshape(n, 3).tolist(), got[:guard].tolist() + got[-guard:].tolist()
    return got.reshape(n, 3).tolist()


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
@pytest.mark.parametrize("h,w", ((11, 17), (4, 48)))
def test_strides_of_either_sign_zero_and_frames_of_one_buffer(h, w, sb):
    n = 3
    p, c, nx = planes3(n, h, w, sb, seed=2)
    size = p.shape[1]
    ref = want(p, c, nx, h, w, sb)
    wide, wider = size + 6 * sb, 2 * size + 16          # beyond a plane: a ragged gap, and one that keeps the planes' alignment
    for sp, sc, sn in ((wide, wider, size), (wider, -wide, -size), (-wider, -wide, wide), (-size, size, -wider)):
        placed = [spread(x, s, f) for x, s, f in ((p, sp, 16), (c, sc, 32), (nx, sn, 48))]
        assert raw([b for b, _ in placed], [f for _, f in placed], (sp, sc, sn), n, h, w, sb) == ref, (sp, sc, sn)
    # stride 0: one plane of an operand against the three of the others
    for which in range(3):
        ops, strides, placed = [p, c, nx], [wide, -wide, wider], []
        ops[which], strides[which] = ops[which][1:2], 0
        for x, s in zip(ops, strides):
            placed.append(spread(x, s, 16))
        assert raw([b for b, _ in placed], [f for _, f in placed], strides, n, h, w, sb) == want(*ops, h, w, sb), which
    # through the binding: an expanded row, and frames i - 1, i, i + 1 of one buffer
    tp, tc, tn = on_device(p), on_device(c), on_device(nx)
    assert sums(tp[0:1].expand(n, size), tc, tn, h, w, sb) == want(p[0:1], c, nx, h, w, sb)
    five = on_device(np.concatenate([p, c[:2]]))
    host = np.concatenate([p, c[:2]])
    assert sums(five[:-2], five[1:-1], five[2:], h, w, sb) == want(host[:-2], host[1:-1], host[2:], h, w, sb)


def test_the_overflow_bound_on_a_full_workgroups_share():
    """Words, two workgroups of 256 whole units each.  Rows of c alternating 0 and 0xFFFF against p = n = 0: every sample of every row adds
    131070 to D, a workgroup's D is 8 * 2048 * 131070 = 2147450880, the bound of the 32-bit partials.  Then c = 0 against p = 0xFFFF on the
    even rows and n = 0xFFFF on the odd ones: the same for A0.  Bytes likewise, far below it."""
    h, w = 2 + 2 * BAND, 8 * GROUP
    for sb, peak in ((2, 0xFFFF), (1, 0xFF)):
        dt = "<u2" if sb == 2 else np.uint8
        zero = np.zeros((2, h, w), dt)
        comb = zero.copy()
        comb[:, 1::2] = peak
        as_bytes = lambda x: np.ascontiguousarray(x).view(np.uint8).reshape(2, -1)  # noqa: E731
        each = 2 * peak * w
        if sb == 2:
            assert BAND * each == 2147450880
        got = sums(on_device(as_bytes(zero)), on_device(as_bytes(comb)), on_device(as_bytes(zero)), h, w, sb)
        assert got == want(as_bytes(zero), as_bytes(comb), as_bytes(zero), h, w, sb) == [[BAND * each, BAND * each, 2 * BAND * each]] * 2
        even, odd = zero.copy(), zero.copy()
        even[:, 0::2], odd[:, 1::2] = peak, peak
        got = sums(on_device(as_bytes(even)), on_device(as_bytes(zero)), on_device(as_bytes(odd)), h, w, sb)
        assert got == want(as_bytes(even), as_bytes(zero), as_bytes(odd), h, w, sb) == [[2 * BAND * each, 0, 0]] * 2


@pytest.mark.parametrize("sb", (1, 2))
def test_words_around_sums_stay_and_two_runs_agree(sb):
    h, w, n = 37, 53, 3
    p, c, nx = planes3(n, h, w, sb, seed=3)
    bufs = [on_device(x) for x in (p, c, nx)]
    size = p.shape[1]
    first, guards = raw(bufs, (0, 0, 0), (size,) * 3, n, h, w, sb, guard=2)
    assert guards == [2 ** 64 - 1] * 4, "the words before and behind sums are not the entry's"
    assert first == want(p, c, nx, h, w, sb)
    assert raw(bufs, (0, 0, 0), (size,) * 3, n, h, w, sb) == first
    assert raw(bufs, (0, 0, 0), (0, 0, 0), 1, 2, w, sb, guard=1) == ([[0, 0, 0]], [2 ** 64 - 1] * 2), "H < 3: the clear alone"


def test_refusals_queue_nothing():
    """Every SSM_E_ARG of the entry with its message, on device memory: `sums` keeps its poison, not even the clear is queued."""
    from ssm_amd import hipbind as hb
    lib = hb.load()
    buf = torch.zeros(3, 256, dtype=torch.uint8, device=DEV)
    out = torch.full((8,), -1, dtype=torch.int64, device=DEV)
    P, C, N, S = buf[0].data_ptr(), buf[1].data_ptr(), buf[2].data_ptr(), out.data_ptr()
    for args, message in [
        ((None, C, N, 64, 64, 64, 1, 8, 8, 1, S), "field_order_sums: null pointer"),
        ((P, C, N, 64, 64, 64, 1, 8, 8, 1, None), "field_order_sums: null pointer"),
        ((P, C, N, 64, 64, 64, 0, 8, 8, 1, S), "field_order_sums: N=0 outside 1..65535"),
        ((P, C, N, 64, 64, 64, 1, 8, 0, 1, S), "field_order_sums: bad plane size 8x0"),
        ((P, C, N, 64, 64, 64, 1, 8, 8, 4, S), "field_order_sums: sample_bytes 4 not in {1, 2}"),
        ((P, C, N, 64, 63, 64, 2, 8, 8, 1, S), "field_order_sums: strides 64 (p), 63 (c), 64 (n) neither 0 nor at least the plane's 64 bytes"),
        ((P, C + 1, N, 128, 128, 128, 2, 8, 8, 2, S), "field_order_sums: a payload of 2-byte samples (p, c or n) is not 2-byte aligned"),
        ((P, C, N, 128, 129, 128, 2, 8, 8, 2, S), "field_order_sums: strides 128 (p), 129 (c), 128 (n) of 2-byte samples must be even"),
        ((P, C, N, 64, 64, 64, 2, 8, 8, 1, S + 4), "field_order_sums: sums is not 8-byte aligned"),
        ((P, C, N, 0, 0, 0, 1, 2147483647, 17, 1, S), "field_order_sums: a plane of 36507221999 bytes is more than the grid takes"),
    ]:
        assert lib.ssm_field_order_sums_fwd(*args, hb.stream_ptr()) == -1
        assert lib.ssm_last_error_string().decode() == message
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -1).all()


# ---- FieldOrderSource ------------------------------------------------------------------------------------------------------------------------
RATE = (30, 1)
H, W = 128, 64          # frames of two 64 x 64 fields: the sizes of tests/test_hip_video_deinterlace.py


def y4m(payloads, tag, interlace, h=H, w=W):
    v = V()
    buf = io.BytesIO()
    with v.Y4MWriter(buf, w, h, rate=RATE, aspect=(1, 1), chroma=tag, interlace=interlace, extended=True) as wr:
        for p in payloads:
            wr.write_frame(p)
    return io.BytesIO(buf.getvalue())


def drain(src):
    out, buf = [], np.empty(src.frame_bytes, np.uint8)
    while src.read_frame_into(buf):
        out.append(buf.copy())
    return np.stack(out)


@pytest.mark.parametrize("tag", ("420jpeg", "422p10"))
def test_source_kinds_verdict_and_bytes_do_not_depend_on_the_chunk(tag):
    v = V()
    bits = v.EXTENDED_TAGS[tag][1]
    for kind, verdict in (("tff", "tff"), ("bff", "bff"), ("progressive", "progressive"), ("still", None)):
        pay = FC.payloads(kind, 7, H, W, tag)
        ref = v.FieldVerdict.of_sums(v.field_order_sums_host(pay[:-2], pay[1:-1], pay[2:], H, W, bits))
        for probe, inner in ((48, 5), (7, 5), (5, 3), (3, 1), (2, 0), (1, 0)):
            for rows in (1, 3, 8):
                src = v.FieldOrderSource(v.Y4MReader(y4m(pay, tag, "p"), extended=True), DEV, probe=probe, frames_per_chunk=rows)
                assert src.decide() == (verdict if inner else None), (kind, probe, rows)
                assert src.kinds == ref.kinds[:inner] and src.counts == tuple(src.kinds.count(k) for k in "TBPU")
                assert all(str(n) in src.note for n in src.counts) and src.interlace == "p"
                assert np.array_equal(drain(src), pay), "the bytes handed out are the reader's, probed or not"
                assert src.frames_read == 7


# ---- VideoInterpolator(field_probe=) ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    return synthetic_model(DEV)


def run(m, cfg, payloads, tag, interlace, rate=2, **kw):
    """(the interpolator after the run, the frames it wrote)."""
    v = V()
    r = v.Y4MReader(y4m(payloads, tag, interlace), extended=True, interlaced=kw.get("deinterlace") is not None)
    sink = io.BytesIO()
    wr = v.Y4MWriter.like(sink, r, rate=v.output_rate(r.rate, rate))
    vi = v.VideoInterpolator(m, cfg, **kw)
    count = vi.run(r, wr)
    assert count == wr.frames_written
    return vi, frames_of(sink.getvalue())


@pytest.fixture(scope="module")
def named(model):
    """Per (tag, order the clip was made in): the clip and what deinterlace=<that order> writes for it: computed once."""
    cfg, m = model
    out = {}
    for tag in ("420jpeg", "422p10"):
        for order in ("tff", "bff"):
            pay = FC.payloads(order, 6, H, W, tag)
            out[tag, order] = pay, run(m, cfg, pay, tag, "p", deinterlace=order)[1]
    return out


@pytest.mark.parametrize("tag", ("420jpeg", "422p10"))
@pytest.mark.parametrize("order", ("tff", "bff"))
def test_auto_on_an_ip_header_equals_the_order_given_by_name(model, named, tag, order):
    cfg, m = model
    pay, want_frames = named[tag, order]
    vi, got = run(m, cfg, pay, tag, "p", deinterlace="auto", field_probe=True)          # a probe longer than the clip
    assert got.shape[0] == 12 and np.array_equal(got, want_frames)
    fp = vi.field_probe
    assert (fp.verdict, fp.order, fp.warning, fp.advice) == (order, order, None, None)
    assert fp.counts == ((4, 0, 0, 0) if order == "tff" else (0, 4, 0, 0)) and fp.kinds == ("T" if order == "tff" else "B") * 4
    assert "4 top field first" in fp.note or "4 bottom field first" in fp.note


@pytest.mark.parametrize("order", ("tff", "bff"))
def test_a_probe_shorter_than_the_clip(model, named, order):
    cfg, m = model
    pay, want_frames = named["420jpeg", order]
    vi, got = run(m, cfg, pay, "420jpeg", "?", deinterlace="auto", field_probe=4)
    assert np.array_equal(got, want_frames) and len(vi.field_probe.kinds) == 2 and vi.field_probe.order == order


def test_progressive_clips_and_stills_are_refused_with_the_counts(model):
    cfg, m = model
    v = V()
    for kind, said, counts in (("progressive", "the clip is progressive", "0 top field first, 0 bottom field first, 4 progressive, 0 undetermined"),
                               ("still", "nothing", "0 top field first, 0 bottom field first, 0 progressive, 4 undetermined")):
        pay = FC.payloads(kind, 6, H, W)
        r = v.Y4MReader(y4m(pay, "420jpeg", "p"), extended=True, interlaced=True)
        sink = io.BytesIO()
        wr = v.Y4MWriter.like(sink, r)
        head = len(sink.getvalue())
        with pytest.raises(ValueError) as e:
            v.VideoInterpolator(m, cfg, deinterlace="auto", field_probe=True).run(r, wr)
        text = str(e.value)
        assert 'deinterlace="auto" on a header that says Ip' in text and said in text and counts in text
        assert 'give deinterlace="tff" or "bff"' in text
        assert len(sink.getvalue()) == head and wr.frames_written == 0, "no frame was written"
    # two frames: no inner frame, no verdict
    with pytest.raises(ValueError, match="the probe says nothing"):
        run(m, cfg, FC.payloads("tff", 2, H, W), "420jpeg", "p", deinterlace="auto", field_probe=True)
    # and without the option the refusal is the one it was
    with pytest.raises(ValueError, match='deinterlace="auto" takes the field order from the Y4M header, and this one says Ip'):
        run(m, cfg, FC.payloads("tff", 3, H, W), "420jpeg", "p", deinterlace="auto")


def test_a_header_that_names_the_order_wins_and_the_disagreement_is_noted(model, named):
    cfg, m = model
    pay, _ = named["420jpeg", "bff"]
    _, as_tff = run(m, cfg, pay, "420jpeg", "p", deinterlace="tff")
    vi, got = run(m, cfg, pay, "420jpeg", "t", deinterlace="auto", field_probe=True)
    assert np.array_equal(got, as_tff), "It over bff data runs as tff"
    fp = vi.field_probe
    assert (fp.verdict, fp.order) == ("bff", "tff") and "the data says bff, the run is tff as the header (It) says; nothing changes" in fp.warning
    vi, got = run(m, cfg, pay, "420jpeg", "p", deinterlace="tff", field_probe=True)
    assert np.array_equal(got, as_tff) and "the run is tff as the option says" in vi.field_probe.warning
    vi, _ = run(m, cfg, pay[:3], "420jpeg", "b", deinterlace="auto", field_probe=True)
    assert vi.field_probe.warning is None and vi.field_probe.order == "bff"


def test_a_report_only_run_writes_what_the_run_without_the_option_writes(model, named):
    cfg, m = model
    pay, _ = named["420jpeg", "tff"]
    vi0, plain = run(m, cfg, pay, "420jpeg", "p", upsample_rate=2)
    vi, got = run(m, cfg, pay, "420jpeg", "p", upsample_rate=2, field_probe=True)
    assert vi0.field_probe is None and got.shape[0] == 11 and np.array_equal(got, plain)
    fp = vi.field_probe
    assert (fp.verdict, fp.order, fp.warning) == ("tff", None, None) and "--deinterlace tff" in fp.advice
    vi, _ = run(m, cfg, FC.payloads("progressive", 4, H, W), "420jpeg", "p", upsample_rate=2, field_probe=3)
    assert (vi.field_probe.verdict, vi.field_probe.advice, vi.field_probe.kinds) == ("progressive", None, "P")


def test_a_telecine_source_is_refused_by_name(model):
    cfg, m = model
    v = V()
    r = v.TelecineSource(v.Y4MReader(y4m(FC.payloads("progressive", 6, H, W), "420jpeg", "p"), extended=True, interlaced=True), DEV)
    with pytest.raises(ValueError, match="field_probe together with detelecine is not available: a telecined clip is a mixture"):
        v.VideoInterpolator(m, cfg, upsample_rate=2, field_probe=True).run(r, v.Y4MWriter.like(io.BytesIO(), r))
