"""Interlaced clips without a GPU: the reader's `interlaced` option, the two numpy yardsticks the kernels are held to
(split_fields_host, weave_fields_host) against a per-row Python loop and hand-written planes, the field timeline (field_of,
field_outputs, the header's rate), and every refused combination of options, in the class and on the command line."""
import io
import re

import numpy as np
import pytest

from ssm_amd import video as V

LAYOUTS = (V.CENTRED, V.COSITED, V.C444, V.C422)
TODAY = "interlaced Y4M input (I%s) is not supported: deinterlace first"


def header(interlace="t", h=8, w=6, chroma="420jpeg", rate="25:1"):
    return io.BytesIO(("YUV4MPEG2 W%d H%d F%s I%s A1:1 C%s\n" % (w, h, rate, interlace, chroma)).encode())


# ---- the reader -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,order", [("t", "tff"), ("b", "bff")])
def test_reader_takes_interlaced_headers_only_when_asked(tag, order):
    r = V.Y4MReader(header(tag), interlaced=True)
    assert r.interlace == tag and r.field_order == order and r.interlaced
    assert r.frame_bytes == 8 * 6 * 3 // 2 and r.field_bytes == V.frame_bytes(4, 6, V.CENTRED) == r.frame_bytes // 2
    with pytest.raises(V.Y4MError) as e:
        V.Y4MReader(header(tag))
    assert str(e.value) == TODAY % tag, "the default refusal is today's text"
    with pytest.raises(V.Y4MError) as e:
        V.Y4MReader(header(tag), extended=True)
    assert str(e.value) == TODAY % tag


def test_reader_progressive_headers_are_as_ever():
    for tag in ("p", "?"):
        for on in (False, True):
            r = V.Y4MReader(header(tag), interlaced=on)
            assert r.field_order is None and r.field_bytes is None and r.frame_bytes == 72


@pytest.mark.parametrize("on", [False, True])
@pytest.mark.parametrize("tag", ["m", "x", "tt"])
def test_reader_refuses_mixed_and_unknown(tag, on):
    with pytest.raises(V.Y4MError) as e:
        V.Y4MReader(header(tag), interlaced=on)
    assert str(e.value) == TODAY % tag


def test_reader_refuses_heights_that_have_no_fields():
    with pytest.raises(V.Y4MError, match=r"interlaced Y4M input \(It\) has an even number of rows: H=7 is odd"):
        V.Y4MReader(header("t", h=7, chroma="444"), interlaced=True)
    with pytest.raises(V.Y4MError, match=r"interlaced Y4M input \(Ib\) in 4:2:0 has a multiple of 4 rows, two chroma fields of H/4: H=6 is not"):
        V.Y4MReader(header("b", h=6), interlaced=True)
    with pytest.raises(V.Y4MError, match="multiple of 4 rows"):
        V.Y4MReader(header("t", h=6, chroma="420mpeg2"), interlaced=True)
    for chroma in ("444", "422", "422p10"):
        r = V.Y4MReader(header("t", h=6, chroma=chroma), extended=True, interlaced=True)
        assert r.field_bytes == V.frame_bytes(3, 6, r.siting, r.bits)
    assert V.Y4MReader(header("p", h=7)).frame_bytes == V.frame_bytes(7, 6, V.CENTRED), "a progressive clip of any height, as ever"


# ---- the yardsticks ---------------------------------------------------------------------------------------------------------------------
def planes_of(h, w, layout):
    ch, cw = V.chroma_dims(h, w, layout)
    return [(h, w), (ch, cw), (ch, cw)]


def loop_split(frames, h, w, layout, sb):
    """Row by row, in samples: field (2n + q) takes rows q, q + 2, ... of every plane of frame n."""
    dt = np.uint8 if sb == 1 else np.dtype("<u2")
    out = []
    for fr in frames:
        x = fr.view(dt)
        for q in (0, 1):
            rows, at = [], 0
            for ph, pw in planes_of(h, w, layout):
                for y in range(ph):
                    if y % 2 == q:
                        rows.append(x[at + y * pw:at + (y + 1) * pw])
                at += ph * pw
            out.append(np.concatenate(rows).view(np.uint8))
    return np.stack(out)


def loop_weave(kept, made, h, w, layout, sb, parity0, fill):
    dt = np.uint8 if sb == 1 else np.dtype("<u2")
    out = []
    for n in range(len(kept)):
        own = (parity0 + n) & 1
        k, m = kept[n].view(dt), (None if fill else made[n].view(dt))
        rows, at = [], 0          # at: the plane's first sample in a FIELD payload
        for ph, pw in planes_of(h, w, layout):
            def field_row(x, r):
                return [int(v) for v in x[at + r * pw:at + (r + 1) * pw]]
            for y in range(ph):
                if y % 2 == own:
                    rows.append(field_row(k, y // 2))
                elif not fill:
                    rows.append(field_row(m, y // 2))
                else:
                    ya, yb = y - 1, y + 1
                    if ya < 0:
                        ya = yb
                    if yb >= ph:
                        yb = ya
                    rows.append([(a + b + 1) >> 1 for a, b in zip(field_row(k, ya // 2), field_row(k, yb // 2))])
            at += (ph // 2) * pw
        out.append(np.array([v for r in rows for v in r], dtype=dt).view(np.uint8))
    return np.stack(out)


def random_bytes(n, count, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(n, count)).astype(np.uint8)


@pytest.mark.parametrize("sb", [1, 2])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("h,w", [(4, 1), (8, 5), (12, 6)])
def test_yardsticks_equal_a_per_row_loop_and_invert_each_other(h, w, layout, sb):
    bits = 8 if sb == 1 else 16
    frames = random_bytes(3, V.frame_bytes(h, w, layout, bits), 100 * h + w + layout + sb)
    fields = V.split_fields_host(frames, h, w, layout, bits)
    assert fields.shape == (6, V.frame_bytes(h // 2, w, layout, bits)) and fields.dtype == np.uint8
    assert np.array_equal(fields, loop_split(frames, h, w, layout, sb))
    other = random_bytes(3, fields.shape[1], 7)
    for parity0 in (0, 1):
        for fill in (0, 1):
            kept = fields[1:4]          # any field payloads: the parity of the rows they land on alternates from parity0
            got = V.weave_fields_host(kept, None if fill else other, h, w, layout, bits, parity0, fill)
            assert got.shape == frames.shape
            assert np.array_equal(got, loop_weave(kept, other, h, w, layout, sb, parity0, fill)), (parity0, fill)
    # weave(split(x)) = x: frame n from its own two fields, the top one kept
    tops, bottoms = fields[0::2], fields[1::2]
    for n in range(3):
        assert np.array_equal(V.weave_fields_host(tops[n:n + 1], bottoms[n:n + 1], h, w, layout, bits, V.TOP, 0)[0], frames[n])
        assert np.array_equal(V.weave_fields_host(bottoms[n:n + 1], tops[n:n + 1], h, w, layout, bits, V.BOTTOM, 0)[0], frames[n])


def test_yardsticks_refuse_heights_without_fields():
    with pytest.raises(V.Y4MError, match="even number of rows"):
        V.split_fields_host(np.zeros((1, 9), np.uint8), 3, 1, V.C444)
    with pytest.raises(V.Y4MError, match="multiple of 4 rows"):
        V.split_fields_host(np.zeros((1, 3), np.uint8), 2, 1, V.CENTRED)
    assert V.split_fields_host(np.zeros((1, 6), np.uint8), 2, 1, V.C444).shape == (2, 3)


def luma_444(rows, dt):
    """A 4:4:4 field of 1-sample-wide planes: the same column for Y, U and V."""
    col = np.array(rows, dtype=dt)
    return np.concatenate([col, col, col]).view(np.uint8)[None]


@pytest.mark.parametrize("bits,lo,hi", [(8, 254, 255), (16, 65534, 65535)])
def test_line_averages_by_hand(bits, lo, hi):
    """A 4-row plane, one sample wide.  Kept top field (rows 0, 2) = (a, b): row 1 = (a + b + 1) >> 1, row 3 has no row 4: both
    neighbours are row 2.  Kept bottom field (rows 1, 3) = (a, b): row 0 has no row -1: both are row 1; row 2 = (a + b + 1) >> 1."""
    dt = np.uint8 if bits == 8 else np.dtype("<u2")

    def column(kept, parity0):
        return V.weave_fields_host(luma_444(kept, dt), None, 4, 1, V.C444, bits, parity0, 1)[0].view(dt)[:4].tolist()

    assert column([0, 1], V.TOP) == [0, 1, 1, 1], "0 + 1 rounds up"
    assert column([0, 1], V.BOTTOM) == [0, 0, 1, 1]
    assert column([lo, hi], V.TOP) == [lo, hi, hi, hi], "the sum needs one bit more than a sample"
    assert column([lo, hi], V.BOTTOM) == [lo, lo, hi, hi]
    assert column([10, 20], V.TOP) == [10, 15, 20, 20] and column([10, 20], V.BOTTOM) == [10, 10, 15, 20]
    assert column([7, 4], V.TOP) == [7, 6, 4, 4]
    # 4:2:0 at H = 4: the chroma fields have one row each, so a missing chroma row has both neighbours clamped onto it
    kept = np.array([1, 2, 3, 4, 50, 60], dtype=dt).view(np.uint8)[None]          # Y 2 x 2, U 1 x 1, V 1 x 1
    got = V.weave_fields_host(kept, None, 4, 2, V.CENTRED, bits, V.BOTTOM, 1)[0].view(dt).tolist()
    assert got == [1, 2, 1, 2, 2, 3, 3, 4, 50, 50, 60, 60]


# ---- the field timeline -----------------------------------------------------------------------------------------------------------------
def test_which_field_is_which_time():
    T, B = V.TOP, V.BOTTOM
    assert [V.field_of(f, "tff") for f in range(4)] == [(0, T), (0, B), (1, T), (1, B)]
    assert [V.field_of(f, "bff") for f in range(4)] == [(0, B), (0, T), (1, B), (1, T)]
    assert V.FIELD_ORDERS == {"t": "tff", "b": "bff"}


@pytest.mark.parametrize("order", ["tff", "bff"])
@pytest.mark.parametrize("n", [1, 2, 5])
def test_outputs_and_the_pairs_that_run(n, order):
    outs = V.field_outputs(n, order)
    assert len(outs) == 2 * n
    for f, (kept, left, right) in enumerate(outs):
        assert kept == V.field_of(f, order)
        if f in (0, 2 * n - 1):
            assert left is None and right is None, "the clip's first and last output are filled"
        else:
            assert left == V.field_of(f - 1, order) and right == V.field_of(f + 1, order)
            assert left[1] == right[1] == 1 - kept[1], "the pair has the missing rows' parity"
            assert right[0] == left[0] + 1, "and is a pair of neighbouring frames of one parity stream"
    if n == 1:
        assert outs == [(V.field_of(0, order), None, None), (V.field_of(1, order), None, None)]
    # per parity stream the pairs that run are every pair of neighbouring frames, once: the fixed grid of upsample_rate = 2 on the sub-clip
    for q in (V.TOP, V.BOTTOM):
        ran = [(left[0], right[0]) for _, left, right in outs if left is not None and left[1] == q]
        assert ran == [(m, m + 1) for m in range(n - 1)]


def test_output_header_rate():
    for rate, want in (((25, 1), (50, 1)), ((30000, 1001), (60000, 1001)), ((50, 1), (100, 1))):
        assert V.output_rate(rate, 2) == want


# ---- refused combinations -------------------------------------------------------------------------------------------------------------
class _Cfg:
    def getint(self, section, key):
        return 2


class _Recurrent:
    recurrent = True


@pytest.mark.parametrize("kw,named", [(dict(upsample_rate=2), "upsample_rate"), (dict(upsample_rate=8), "upsample_rate"),
                                      (dict(target_rate=(60, 1)), "target_rate"), (dict(speed="1/2"), "speed"),
                                      (dict(speed=1, shutter="1/2"), "speed"), (dict(scene_cut="1/10"), "scene_cut")])
def test_refused_option_pairs(kw, named):
    with pytest.raises(ValueError, match="deinterlace together with %s is not available" % named):
        V.VideoInterpolator(None, _Cfg(), deinterlace="auto", **kw)


def test_refused_shutter_recurrent_and_unknown_values():
    with pytest.raises(ValueError, match="deinterlace together with shutter is not available"):
        V.VideoInterpolator(None, _Cfg(), deinterlace="tff", shutter="1/2")
    with pytest.raises(ValueError, match="deinterlace together with a recurrent model is not available"):
        V.VideoInterpolator(_Recurrent(), _Cfg(), deinterlace="bff")
    with pytest.raises(ValueError, match="unknown deinterlace 'yes': it is one of auto, tff, bff"):
        V.VideoInterpolator(None, _Cfg(), deinterlace="yes")
    for ok in ("auto", "tff", "bff"):
        vi = V.VideoInterpolator(None, _Cfg(), deinterlace=ok, matrix=V.BT709, color_range=V.FULL, flow_scale=2)
        assert vi.deinterlace == ok
        assert V.VideoInterpolator(None, _Cfg(), deinterlace=ok, tile=(64, 64), halo=32, blend=8).tile == (64, 64)
    vi = V.VideoInterpolator(None, _Cfg())
    assert vi.deinterlace is None and vi.rate == 8, "without the option nothing changes"


def test_field_order_of_a_run():
    assert V.field_order("auto", "t") == "tff" and V.field_order("auto", "b") == "bff"
    for tag in ("p", "?", "m"):
        with pytest.raises(ValueError, match=re.escape('deinterlace="auto" takes the field order from the Y4M header, and this one says I%s' % tag)):
            V.field_order("auto", tag)
        assert V.field_order("tff", tag) == "tff" and V.field_order("bff", tag) == "bff"
    assert V.field_order("bff", "t") == "bff", "tff / bff override any header"


# ---- command line -----------------------------------------------------------------------------------------------------------------------
BASE = ["-c", "x.ini", "--expt", "e", "--log", "l", "--input", "-", "--output", "-"]


def test_cli_flag():
    import interpolate_video as cli
    a = cli.getargs(BASE)
    assert a.deinterlace is None and a.upsample_rate == 8, "without the flag the tool is as it was"
    for mode in ("auto", "tff", "bff"):
        a = cli.getargs(BASE + ["--deinterlace", mode])
        assert a.deinterlace == mode and a.upsample_rate is None and a.fps is None and not a.slowmo
    a = cli.getargs(BASE + ["--deinterlace", "auto", "--matrix", "bt709", "--range", "full", "--flow_scale", "2"])
    assert a.deinterlace == "auto" and a.matrix == "bt709" and a.flow_scale == 2
    assert cli.getargs(BASE + ["--deinterlace", "tff", "--tile", "64x64"]).tile == (64, 64)


@pytest.mark.parametrize("extra,named", [(["--upsample_rate", "2"], "--upsample_rate"), (["--slowmo"], "--slowmo"), (["--fps", "60"], "--fps"),
                                         (["--speed", "1/2"], "--speed"), (["--speed", "1", "--shutter", "180"], "--speed"),
                                         (["--shutter", "180"], "--shutter"), (["--scene_cut", "0.1"], "--scene_cut")])
def test_cli_refusals(extra, named, capsys):
    import interpolate_video as cli
    with pytest.raises(SystemExit) as e:
        cli.getargs(BASE + ["--deinterlace", "auto"] + extra)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "--deinterlace does not go together with %s" % named in err


def test_cli_refuses_an_unknown_mode(capsys):
    import interpolate_video as cli
    with pytest.raises(SystemExit) as e:
        cli.getargs(BASE + ["--deinterlace", "yes"])
    assert e.value.code == 2 and "--deinterlace" in capsys.readouterr().err
