"""Blocks that do not change without a GPU: the definition in numpy (static_paste_host) against a loop written out sample by
sample, parse_static, the option refusals of VideoInterpolator and the command line, the lines the tool logs, and every refusal of
ssm_static_paste_fwd through the library as tests/test_cabi_cpu.py loads it."""
import configparser
import os
import sys

import numpy as np
import pytest

from ssm_amd import video as V

LAYOUTS = (V.CENTRED, V.COSITED, V.C422, V.C444)
CHROMA_BLOCK = {V.CENTRED: (4, 4), V.COSITED: (4, 4), V.C422: (8, 4), V.C444: (8, 8)}          # (rows, columns) under an 8 x 8 luma block


def paste_by_loops(outputs, a, b, h, w, layout, bits, lo):
    """The definition of include/ssm_hip.h sample by sample, in Python ints: (outputs with the static blocks of a pasted, counts)."""
    sb = V.sample_bytes(bits)
    ch, cw = V.chroma_dims(h, w, layout)
    cr, cc = CHROMA_BLOCK[layout]
    planes = ((0, w, 8, 8), (h * w, cw, cr, cc), (h * w + ch * cw, cw, cr, cc))          # first sample, row pitch, block rows, block columns

    def sample(p, i):
        return int(p[i]) if sb == 1 else int(p[2 * i]) | int(p[2 * i + 1]) << 8

    res, counts = outputs.copy(), []
    for n in range(a.shape[0]):
        count = 0
        for by in range(h >> 3):
            for bx in range(w >> 3):
                at = [first + (rows * by + r) * pitch + cols * bx + c for first, pitch, rows, cols in planes for r in range(rows)
                      for c in range(cols)]
                d = sum(abs(sample(a[n], i) - sample(b[n], i)) for i in at)
                if d <= lo:
                    count += 1
                    for j in range(outputs.shape[1]):
                        for i in at:
                            res[n, j, sb * i:sb * i + sb] = a[n, sb * i:sb * i + sb]
        counts.append(count)
    return res, counts


def pair_clip(h, w, layout, bits, n=2, t=2, seed=0, extra=0):
    """(outputs [n, t, fb + extra], a, b [n, fb + extra]) of random samples in which about half of the blocks of b are a's, one block differs
    in a single V sample by 1 and one is equal in luma and different in U."""
    rng = np.random.RandomState(seed + 100 * h + w + layout + bits)
    fb = V.frame_bytes(h, w, layout, bits)
    a = rng.randint(0, 256, size=(n, fb + extra)).astype(np.uint8)
    b = rng.randint(0, 256, size=(n, fb + extra)).astype(np.uint8)
    frames_b = np.ascontiguousarray(b[:, :fb])
    pa, pb = (V.split_planes(x, h, w, layout, bits) for x in (np.ascontiguousarray(a[:, :fb]), frames_b))
    cr, cc = CHROMA_BLOCK[layout]
    blocks = [(by, bx) for by in range(h >> 3) for bx in range(w >> 3)]
    for k, (by, bx) in enumerate(blocks):
        if k % 2 == 0 or k < 3:
            for (x, y), (rr, rc) in zip(zip(pa, pb), ((8, 8), (cr, cc), (cr, cc))):
                y[:, rr * by:rr * by + rr, rc * bx:rc * bx + rc] = x[:, rr * by:rr * by + rr, rc * bx:rc * bx + rc]
    if len(blocks) >= 3:
        (by, bx), (cy, cx) = blocks[1], blocks[2]
        pb[2][:, cr * by + cr - 1, cc * bx + cc - 1] ^= 1          # block 1: one V sample, by 1
        pb[1][:, cr * cy, cc * cx] ^= 0x55                         # block 2: luma equal, U different
    b[:, :fb] = frames_b          # the planes are views of it
    outputs = rng.randint(0, 256, size=(n, t, fb + extra)).astype(np.uint8)
    return outputs, a, b


@pytest.mark.parametrize("lo", [0, 1, 37, 5000])
def test_the_yardstick_is_the_definition_written_out(lo):
    h, w, layout, bits = 17, 27, V.CENTRED, 8
    outputs, a, b = pair_clip(h, w, layout, bits, n=2, t=2, seed=lo)
    got, counts = V.static_paste_host(outputs, a, b, h, w, layout, bits, lo)
    want, want_counts = paste_by_loops(outputs, a, b, h, w, layout, bits, lo)
    assert counts.dtype == np.uint64 and counts.tolist() == want_counts
    assert np.array_equal(got, want)
    assert 0 < want_counts[0] < V.static_blocks(h, w) == 6 or lo == 5000
    if lo == 0:
        assert want_counts == [2, 2], "blocks 0 and 4 agree; block 1 differs in one V sample, block 2 in U alone"
    if lo == 1:
        assert want_counts == [3, 3], "the single V sample that differs by 1 is within lo = 1"


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("bits", [8, 10, 16])
def test_the_yardstick_in_every_format(layout, bits):
    h, w = 19, 26
    outputs, a, b = pair_clip(h, w, layout, bits, n=1, t=1, seed=3, extra=5)
    for lo in (0, 300):
        got, counts = V.static_paste_host(outputs, a, b, h, w, layout, bits, lo)
        want, want_counts = paste_by_loops(outputs, a, b, h, w, layout, bits, lo)
        assert counts.tolist() == want_counts and np.array_equal(got, want)
    assert np.array_equal(got[:, :, -5:], outputs[:, :, -5:]), "bytes behind the frame stay"


def test_the_yardstick_on_frames_without_blocks_and_on_equal_frames():
    outputs, a, b = pair_clip(7, 64, V.C444, 8, n=2, t=3)
    got, counts = V.static_paste_host(outputs, a, a, 7, 64, V.C444, 8, 0)
    assert np.array_equal(got, outputs) and counts.tolist() == [0, 0]
    outputs, a, b = pair_clip(27, 45, V.CENTRED, 10, n=2, t=3)
    got, counts = V.static_paste_host(outputs, a, a, 27, 45, V.CENTRED, 10, 0)
    assert counts.tolist() == [15, 15] and V.static_blocks(27, 45) == 15
    fb = V.frame_bytes(27, 45, V.CENTRED, 10)
    gy, oy, ay = (V.split_planes(np.ascontiguousarray(x.reshape(-1, fb)), 27, 45, V.CENTRED, 10)[0] for x in (got, outputs, np.repeat(a, 3, axis=0)))
    assert np.array_equal(gy[:, :24, :40], ay[:, :24, :40]) and np.array_equal(gy[:, 24:], oy[:, 24:]) and np.array_equal(gy[:, :, 40:], oy[:, :, 40:])


def test_parse_static():
    for text, want in ((0, 0), ("0", 0), (" 37 ", 37), (320, 320), (np.int64(5), 5), (2.0, 2), ("16777215", (1 << 24) - 1)):
        got = V.parse_static(text)
        assert got == want and type(got) is int
    assert V.STATIC_MAX == (1 << 24) - 1
    for bad in ("", "x", "1.5", 1.5, -1, "-1", 1 << 24, "16777216", True, None, "0:0", (1, 2)):
        with pytest.raises(ValueError) as e:
            V.parse_static(bad)
        assert repr(bad) in str(e.value) and "2^24 - 1" in str(e.value)


class _Model:
    recurrent = False
    precision = None


class _Recurrent(_Model):
    recurrent = True


def _cfg():
    cfg = configparser.RawConfigParser()
    cfg.read_dict({"TRAIN": {"N_FRAMES": "2"}})
    return cfg


def test_interpolator_takes_the_option_and_refuses_what_does_not_go_with_it():
    vi = V.VideoInterpolator(_Model(), _cfg())
    assert vi.static_lo is None and vi.static == []
    assert V.VideoInterpolator(_Model(), _cfg(), upsample_rate=3, static=0).static_lo == 0
    vi = V.VideoInterpolator(_Model(), _cfg(), target_rate=(60, 1), scene_cut="1/10", flow_scale=2, static="37")
    assert vi.static_lo == 37 and vi.static == []
    assert V.VideoInterpolator(_Model(), _cfg(), speed="1/2", tile=(64, 64), static=320).static_lo == 320
    for name, kw, model in (("shutter", dict(shutter="1/2", speed=1), _Model), ("deinterlace", dict(deinterlace="tff"), _Model),
                            ("dedup", dict(dedup=True), _Model), ("active", dict(active="auto"), _Model),
                            ("a recurrent model", {}, _Recurrent)):
        with pytest.raises(ValueError, match="static together with %s is not available.*chain two runs" % name):
            V.VideoInterpolator(model(), _cfg(), static=0, **kw)
    with pytest.raises(ValueError, match="static.*2\\^24 - 1.*-3"):
        V.VideoInterpolator(_Model(), _cfg(), static=-3)


def _tool():
    scripts = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "superslomo-videointerpolation-pytorch_amd", "scripts")
    if scripts not in sys.path:
        sys.path.insert(0, scripts)
    import interpolate_video
    return interpolate_video


def test_command_line_takes_the_option_and_refuses_what_does_not_go_with_it(capsys):
    tool = _tool()
    base = ["-c", "x.ini", "--expt", "e", "--log", "l", "--input", "-", "--output", "-"]
    assert tool.getargs(base).static is None
    assert tool.getargs(base + ["--static", "0"]).static == 0
    assert tool.getargs(base + ["--static", "320", "--fps", "60", "--scene_cut", "0.1", "--detelecine"]).static == 320
    for flag, extra in (("--shutter", ["--shutter", "180", "--speed", "1/2"]), ("--deinterlace", ["--deinterlace", "tff"]),
                        ("--dedup", ["--dedup"]), ("--active", ["--active", "auto"])):
        with pytest.raises(SystemExit):
            tool.getargs(base + ["--static", "0"] + extra)
        assert "--static does not go together with %s" % flag in capsys.readouterr().err
    with pytest.raises(SystemExit):
        tool.getargs(base + ["--static", "1.5"])
    assert "'1.5'" in capsys.readouterr().err


def test_the_lines_the_tool_logs():
    tool = _tool()
    assert tool.static_lines([], 0) == ["static: lo = 0, no pair got a synthesised frame"]
    assert tool.static_lines([(0, 0, 0), (1, 0, 0)], 5) == ["static: lo = 5, 2 pairs, the frame has no 8 x 8 block: nothing is kept"]
    lines = tool.static_lines([(0, 24, 96), (1, 0, 96), (2, 48, 96)], 0)
    assert lines == ["static: lo = 0, 3 pairs, 72 of 288 blocks kept (25.00%), per pair at most 50.00% and at least 0.00%",
                     "static: no static block between input frames 1 and 2"]
    assert len(tool.static_lines([(0, 0, 96), (1, 0, 96)], 0)) == 1, "no pair had a static block: the summary alone"


# ---- the entry's refusals ------------------------------------------------------------------------------------------------------------------
P, Q, C = 0x10000, 0x90000, 0x70000          # a, out and counts: addresses that are only looked at; b is a + one 16 x 16 4:4:4 frame
FB = 16 * 16 * 3


@pytest.mark.parametrize("args, message", [
    ((0, P, FB, FB, Q, FB, 1, 1, 16, 16, 2, 1, 0, C), "static_paste: null pointer"),
    ((P, 0, FB, FB, Q, FB, 1, 1, 16, 16, 2, 1, 0, C), "static_paste: null pointer"),
    ((P, P, FB, FB, 0, FB, 1, 1, 16, 16, 2, 1, 0, C), "static_paste: null pointer"),
    ((P, P, FB, FB, Q, FB, 1, 1, 16, 16, 2, 1, 0, 0), "static_paste: null pointer"),
    ((P, P, FB, FB, Q, FB, 0, 1, 16, 16, 2, 1, 0, C), "static_paste: N=0 outside 1..65535"),
    ((P, P, FB, FB, Q, FB, 65536, 1, 16, 16, 2, 1, 0, C), "static_paste: N=65536 outside 1..65535"),
    ((P, P, FB, FB, Q, FB, 1, 0, 16, 16, 2, 1, 0, C), "static_paste: T=0 outside 1..65535"),
    ((P, P, FB, FB, Q, FB, 1, 65536, 16, 16, 2, 1, 0, C), "static_paste: T=65536 outside 1..65535"),
    ((P, P, FB, FB, Q, FB, 1, 1, 0, 16, 2, 1, 0, C), "static_paste: bad frame size 0x16"),
    ((P, P, FB, FB, Q, FB, 1, 1, 16, -1, 2, 1, 0, C), "static_paste: bad frame size 16x-1"),
    ((P, P, FB, FB, Q, FB, 1, 1, 16, 16, 4, 1, 0, C), "static_paste: layout 4 not in {0, 1, 2, 3}"),
    ((P, P, FB, FB, Q, FB, 1, 1, 16, 16, -1, 1, 0, C), "static_paste: layout -1 not in {0, 1, 2, 3}"),
    ((P, P, FB, FB, Q, FB, 1, 1, 16, 16, 2, 3, 0, C), "static_paste: sample_bytes 3 not in {1, 2}"),
    ((P, P, FB, FB, Q, FB, 1, 1, 16, 16, 2, 1, 1 << 24, C), "static_paste: lo=16777216 outside 0..2^24-1"),
    ((P, P + FB, FB - 1, FB, Q, FB, 2, 1, 16, 16, 2, 1, 0, C), "static_paste: strides 767 (a), 768 (b) shorter than the frame's 768 bytes"),
    ((P, P + FB, FB, -FB + 1, Q, FB, 2, 1, 16, 16, 2, 1, 0, C), "static_paste: strides 768 (a), -767 (b) shorter than the frame's 768 bytes"),
    ((P, P + FB, 0, FB, Q, FB, 2, 1, 16, 16, 2, 1, 0, C), "static_paste: strides 0 (a), 768 (b) shorter than the frame's 768 bytes"),
    ((P, P + FB, 0, 0, Q, FB - 1, 1, 2, 16, 16, 2, 1, 0, C), "static_paste: stride 767 (out) shorter than the frame's 768 bytes"),
    ((P, P + FB, FB, FB, Q, 0, 2, 1, 16, 16, 2, 1, 0, C), "static_paste: stride 0 (out) shorter than the frame's 768 bytes"),
    ((P + 1, P, 2 * FB, 2 * FB, Q, 2 * FB, 1, 1, 16, 16, 2, 2, 0, C), "static_paste: a payload of 2-byte samples (a, b or out) is not 2-byte aligned"),
    ((P, P, 2 * FB, 2 * FB, Q + 1, 2 * FB, 1, 1, 16, 16, 2, 2, 0, C), "static_paste: a payload of 2-byte samples (a, b or out) is not 2-byte aligned"),
    ((P, P, 2 * FB + 1, 2 * FB, Q, 2 * FB, 2, 1, 16, 16, 2, 2, 0, C),
     "static_paste: strides 1537 (a), 1536 (b), 1536 (out) of 2-byte samples must be even"),
    ((P, P, 2 * FB, 2 * FB, Q, 2 * FB + 1, 2, 1, 16, 16, 2, 2, 0, C),
     "static_paste: strides 1536 (a), 1536 (b), 1537 (out) of 2-byte samples must be even"),
    ((P, P + FB, FB, FB, P + 2 * FB, FB, 2, 2, 16, 16, 2, 1, 0, C), "static_paste: out overlaps a or b"),
    ((P, P + FB, FB, FB, P + FB - 1, -FB, 1, 2, 16, 16, 2, 1, 0, C), "static_paste: out overlaps a or b"),
    ((P, Q, FB, FB, Q + FB - 1, FB, 1, 1, 16, 16, 2, 1, 0, C), "static_paste: out overlaps a or b"),
    ((P, P, FB, FB, Q, FB, 1, 1, 16, 16, 2, 1, 0, C + 4), "static_paste: counts is not 8-byte aligned"),
])
def test_static_paste_refusals(args, message):
    from ssm_amd import hipbind as hb
    lib = hb.load()
    assert lib.ssm_static_paste_fwd(*args, None) == -1
    assert lib.ssm_last_error_string().decode() == message


def test_static_paste_refuses_in_the_order_of_the_header():
    """A call that is wrong in every way is refused for the first reason of the header's list; one that is right up to the overlap is refused
    only for that (nothing is queued by either: no launch on the null stream)."""
    from ssm_amd import hipbind as hb
    lib = hb.load()
    assert lib.ssm_static_paste_fwd(P + 1, P + 1, 1, 1, P + 1, 1, 0, 0, 0, 0, 9, 9, 1 << 24, C + 4, None) == -1
    assert lib.ssm_last_error_string().decode() == "static_paste: N=0 outside 1..65535"
    assert lib.ssm_static_paste_fwd(P + 1, P + 1, 1, 1, P + 1, 1, 2, 2, 16, 16, 2, 2, 1 << 24, C + 4, None) == -1
    assert lib.ssm_last_error_string().decode() == "static_paste: lo=16777216 outside 0..2^24-1"
    assert lib.ssm_static_paste_fwd(P + 1, P + 1, 1, 1, P + 1, 1, 2, 2, 16, 16, 2, 2, 5, C + 4, None) == -1
    assert lib.ssm_last_error_string().decode() == "static_paste: strides 1 (a), 1 (b) shorter than the frame's 1536 bytes"
    # overlapping a and b are fine (frames n and n + 1 of one buffer); out behind them is not
    assert lib.ssm_static_paste_fwd(P, P + FB, FB, FB, P + 3 * FB - 1, FB, 2, 3, 16, 16, 2, 1, 0, C + 4, None) == -1
    assert lib.ssm_last_error_string().decode() == "static_paste: out overlaps a or b"
