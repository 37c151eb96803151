"""The flow check's per-block fallback without a GPU: ssm_amd.video.flow_paste_host against a loop written out block by
block and sample by sample, the rule that says which outputs of a pair take the left frame, the refusals of the option flow_blocks in
VideoInterpolator and in scripts/interpolate_video.py, and the SSM_E_ARG refusals of ssm_flow_paste_fwd, in their order, through the
loaded library.  Everything compared is exact."""
import argparse
import os
import sys
from fractions import Fraction as Fr

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import video_option_cases as C  # noqa: E402
from video_clips import LAYOUTS  # noqa: E402
from ssm_amd import video as V  # noqa: E402

SIZES = ((8, 8), (16, 24), (17, 23), (7, 40), (40, 7))
N, T = 2, 3


# ---- the yardstick against a loop ----------------------------------------------------------------------------------------------------------
def plane_offsets(h, w, layout):
    """(rows, columns, first sample) of Y, U and V in a payload, and the chroma samples (rows, columns) under a luma block."""
    ch, cw = V.chroma_dims(h, w, layout)
    sub = (8, 8) if layout == V.C444 else (8, 4) if layout == V.C422 else (4, 4)
    return ((h, w, 0), (ch, cw, h * w), (ch, cw, h * w + ch * cw)), sub


def by_loop(outputs, a, b, mask, h, w, layout, bits, k, split):
    """The definition, one block and one sample at a time, on the samples as integers."""
    sb = V.sample_bytes(bits)
    fb = V.frame_bytes(h, w, layout, bits)
    res, counts = outputs.copy(), [0] * outputs.shape[0]
    planes, sub = plane_offsets(h, w, layout)
    for n in range(outputs.shape[0]):
        for by in range(h >> 3):
            for bx in range(w >> 3):
                bad = 0
                for y in range(8 * by, 8 * by + 8):
                    for x in range(8 * bx, 8 * bx + 8):
                        bad += (int(mask[n, 0, y, x]) | int(mask[n, 1, y, x])) & 1
                if bad <= k:
                    continue
                counts[n] += 1
                for p, (rows, cols, first) in enumerate(planes):
                    rr, rc = (8, 8) if p == 0 else sub
                    for y in range(rr * by, rr * by + rr):
                        for x in range(rc * bx, rc * bx + rc):
                            o = (first + y * cols + x) * sb
                            assert y < rows and x < cols and o + sb <= fb
                            for j in range(outputs.shape[1]):
                                src = a if j < split else b
                                res[n, j, o:o + sb] = src[n, o:o + sb]
    return res, counts


def planted_mask(h, w, k, seed):
    """[N, 2, h, w] over {0, 1, 2} at random, then, where the frame has them, blocks with a known n: block 0 n = k exactly (direction 0
    alone, the rest of the block `leaves`), block 1 n = k + 1 in direction 1 alone, block 2 inconsistent everywhere in both directions,
    block 3 of bytes 2 alone.  -> (mask, {block: n} of pair 0's planted blocks)."""
    rng = np.random.RandomState(seed)
    mask = rng.randint(0, 3, size=(N, 2, h, w)).astype(np.uint8)
    blocks = [(by, bx) for by in range(h >> 3) for bx in range(w >> 3)]
    planted = {}

    def fill(blk, d0, d1):
        by, bx = blocks[blk]
        for d, count in ((0, d0), (1, d1)):
            flat = np.full(64, 2, np.uint8)
            flat[rng.permutation(64)[:count]] = 1
            mask[:, d, 8 * by:8 * by + 8, 8 * bx:8 * bx + 8] = flat.reshape(8, 8)

    if len(blocks) > 0:
        fill(0, k, 0)
        planted[0] = k
    if len(blocks) > 1:
        fill(1, 0, min(k + 1, 64))
        planted[1] = min(k + 1, 64)
    if len(blocks) > 2:
        fill(2, 64, 64)
        planted[2] = 64
    if len(blocks) > 3:
        fill(3, 0, 0)
        planted[3] = 0
    return mask, planted


def operands(h, w, layout, bits, seed):
    rng = np.random.RandomState(seed)
    fb = V.frame_bytes(h, w, layout, bits)
    a, b = (rng.randint(0, 256, size=(N, fb + 3)).astype(np.uint8) for _ in range(2))
    outputs = rng.randint(0, 256, size=(N, T, fb + 5)).astype(np.uint8)
    return a, b, outputs


@pytest.mark.parametrize("bits", [8, 10, 16])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_yardstick_equals_the_loop(layout, bits):
    for h, w in SIZES:
        a, b, outputs = operands(h, w, layout, bits, seed=h * w + layout + bits)
        for k, split in ((20, 1), (0, 0), (63, T)):
            mask, planted = planted_mask(h, w, k, seed=k + h)
            counts_host = V.flow_block_counts_host(mask, h, w)
            for blk, n in planted.items():
                assert counts_host[0].reshape(-1)[blk] == n, "a pixel inconsistent in both directions counts once, one that leaves nothing"
            got, counts = V.flow_paste_host(outputs, a, b, mask, h, w, layout, bits, k, split)
            want, want_counts = by_loop(outputs, a, b, mask, h, w, layout, bits, k, split)
            assert counts.dtype == np.uint64 and counts.tolist() == want_counts, (h, w, k, split)
            assert np.array_equal(got, want), (h, w, k, split)
            fail = counts_host > k
            if 0 in planted:
                assert not fail[0].reshape(-1)[0], "n = K passes"
            if 1 in planted and k < 64:
                assert fail[0].reshape(-1)[1], "n = K + 1 in direction 1 alone fails"
            if 3 in planted:
                assert not fail[0].reshape(-1)[3], "bytes 2 alone: n = 0"
            if not V.static_blocks(h, w):
                assert np.array_equal(got, outputs) and counts.tolist() == [0, 0], "a frame without blocks"
        mask, _ = planted_mask(h, w, 0, seed=9)
        got, counts = V.flow_paste_host(outputs, a, b, mask, h, w, layout, bits, 64, 1)
        assert np.array_equal(got, outputs) and counts.tolist() == [0, 0], "K = 64 changes nothing"


def test_outputs_left_and_right_of_split_take_their_side():
    h, w, layout, bits = 16, 24, V.CENTRED, 8
    a, b, outputs = operands(h, w, layout, bits, seed=3)
    mask = np.ones((N, 2, h, w), np.uint8)
    fb = V.frame_bytes(h, w, layout, bits)
    got, counts = V.flow_paste_host(outputs, a, b, mask, h, w, layout, bits, 0, 1)
    assert counts.tolist() == [6, 6]
    assert np.array_equal(got[:, 0, :fb], a[:, :fb]) and np.array_equal(got[:, 1, :fb], b[:, :fb]) and np.array_equal(got[:, 2, :fb], b[:, :fb])
    assert np.array_equal(got[:, :, fb:], outputs[:, :, fb:]), "the bytes behind a payload stay"


# ---- which outputs take the left frame ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", range(2, 10))
def test_split_of_the_fixed_grid(rate):
    times = [Fr(j, rate) for j in range(1, rate)]
    assert V.fixed_split(rate) == sum(1 for t in times if t < Fr(1, 2)) == V.times_split(times)
    assert all((t < Fr(1, 2)) == (j < V.fixed_split(rate)) for j, t in enumerate(times))


@pytest.mark.parametrize("target", [(640, 1), (600, 1)])
def test_split_of_a_timeline(target):
    tl = V.Timeline(V.timeline_step((240, 1), target))
    n = 12
    per_pair = {}
    for i, t in tl.outputs(n):
        if t:
            per_pair.setdefault(i, []).append(t)
    assert len(per_pair) > 1
    for i, times in per_pair.items():
        assert times == tl.times(i), "a pair's times as the planner's rows hold them"
        split = V.times_split(times)
        assert [t < Fr(1, 2) for t in times] == [j < split for j in range(len(times))], "t < 1/2: left"
    with pytest.raises(AssertionError, match="ascend"):
        V.times_split([Fr(3, 4), Fr(1, 4)])


# ---- the option's refusals -------------------------------------------------------------------------------------------------------------------
def api(**kw):
    return V.VideoInterpolator(C._Model(), C._cfg(), **kw)


def test_the_option_is_no_row_of_the_table():
    assert "flow_blocks" not in V.OPTIONS and "flow_blocks" not in V.OPTION_RULES


def test_video_interpolator_refuses():
    with pytest.raises(ValueError) as e:
        api(flow_blocks=3)
    assert str(e.value) == "flow_blocks is the flow check's per-block fallback: give flow_check, or leave it out"
    with pytest.raises(ValueError, match="^flow_blocks together with active is not available.*chain two runs$"):
        api(flow_check=True, flow_blocks=3, active="auto")
    for bad in (-1, 65, 1.5, True, "x"):
        with pytest.raises(ValueError, match=r"^flow_blocks, .* whole number in 0 \.\. 64 \(got"):
            api(flow_check=True, flow_blocks=bad)
    for k in (0, 64, "17"):
        assert api(flow_check=True, flow_blocks=k).flow_blocks == int(k)
    vi = api(flow_check="1/2", flow_blocks=5, static=0, scene_cut="1/10")
    assert vi.flow_blocks == 5 and vi.flow_repaired == []
    assert api(flow_check=True).flow_blocks is None
    # what the flow check refuses stays the table's refusal, as recorded: the table speaks first
    with pytest.raises(ValueError) as e:
        api(flow_check=True, flow_blocks=3, tile=(64, 64))
    assert str(e.value) == C.api_outcome(V, ("flow_check", "tile"))[1]


def tool_refusal(words):
    import interpolate_video

    class Refused(Exception):
        pass

    def error(self, message):
        raise Refused(message)

    kept, argparse.ArgumentParser.error = argparse.ArgumentParser.error, error
    try:
        return vars(interpolate_video.getargs(C.BASE + words))
    except Refused as e:
        return str(e)
    finally:
        argparse.ArgumentParser.error = kept


def test_the_tool_refuses():
    assert tool_refusal(["--flow_blocks", "3"]) == "--flow_blocks is --flow_check's per-block fallback: it needs --flow_check"
    text = tool_refusal(["--flow_check", "--flow_blocks", "3", "--active", "auto"])
    assert text.startswith("--flow_blocks does not go together with --active") and text.endswith("chain two runs")
    for bad in ("-1", "65", "1.5"):
        text = tool_refusal(["--flow_check", "--flow_blocks", bad])
        assert text.startswith("argument --flow_blocks: --flow_blocks, ") and "0 .. 64 (got %r)" % bad in text, text
    args = tool_refusal(["--flow_check", "--flow_blocks", "12"])
    assert args["flow_blocks"] == 12 and args["flow_check"] == (None, None, None)
    assert tool_refusal(["--flow_check", "--flow_blocks", "3", "--tile", "64x64"]) == C.flag_outcome(
        __import__("interpolate_video"), ("flow_check", "tile"))
    assert tool_refusal([])["flow_blocks"] is None


def test_the_log_lines():
    import interpolate_video as tool
    assert tool.flow_blocks_lines([], 5) == ["flow blocks: K = 5, no pair got a synthesised frame"]
    assert tool.flow_blocks_lines([(0, 0, 0)], 5) == ["flow blocks: K = 5, 1 pairs, the frame has no 8 x 8 block: nothing is replaced"]
    lines = tool.flow_blocks_lines([(0, 24, 96), (1, 96, 96), (2, 0, 96)], 5)
    assert lines == ["flow blocks: K = 5, 3 pairs, 120 of 288 blocks replaced (41.67%), per pair at most 100.00% and at least 0.00%",
                     "flow blocks: every block failed between input frames 1 and 2"]


# ---- the entry's refusals, through the library -------------------------------------------------------------------------------------------
def entry_cases():
    """(what is broken, the arguments, the message): one valid set at 16 x 24, 4:2:0, bytes, N = 2, T = 3 on made-up addresses, one
    thing broken per case; where two things are broken the earlier one of the header's order speaks."""
    fb = V.frame_bytes(16, 24, V.CENTRED, 8)
    ok = dict(a=0x10000, b=0x20000, sa=fb, sb=fb, out=0x40000, so=fb, N=2, T=3, split=1, H=16, W=24, layout=0, sbytes=1, mask=0x80000,
              sm=2 * 16 * 24, K=8, counts=0x90000)
    rows = [
        ("null a", dict(a=None), "flow_paste: null pointer"),
        ("null mask", dict(mask=None), "flow_paste: null pointer"),
        ("null counts", dict(counts=None), "flow_paste: null pointer"),
        ("N = 0", dict(N=0), "flow_paste: N=0 outside 1..65535"),
        ("N = 0 and T = 0", dict(N=0, T=0), "flow_paste: N=0 outside 1..65535"),
        ("T = 65536", dict(T=65536), "flow_paste: T=65536 outside 1..65535"),
        ("split = -1", dict(split=-1), "flow_paste: split=-1 outside 0..T=3"),
        ("split = 4", dict(split=4), "flow_paste: split=4 outside 0..T=3"),
        ("split = 4 and H = 0", dict(split=4, H=0), "flow_paste: split=4 outside 0..T=3"),
        ("H = 0", dict(H=0), "flow_paste: bad frame size 0x24"),
        ("H = 0 and layout = 4", dict(H=0, layout=4), "flow_paste: bad frame size 0x24"),
        ("layout = 4", dict(layout=4), "flow_paste: layout 4 not in {0, 1, 2, 3}"),
        ("layout = 4 and sample_bytes = 3", dict(layout=4, sbytes=3), "flow_paste: layout 4 not in {0, 1, 2, 3}"),
        ("sample_bytes = 3", dict(sbytes=3), "flow_paste: sample_bytes 3 not in {1, 2}"),
        ("sample_bytes = 3 and K = 65", dict(sbytes=3, K=65), "flow_paste: sample_bytes 3 not in {1, 2}"),
        ("K = 65", dict(K=65), "flow_paste: K=65 outside 0..64"),
        ("K = -1", dict(K=-1), "flow_paste: K=-1 outside 0..64"),
        ("K = 65 and a short stride of a", dict(K=65, sa=fb - 1), "flow_paste: K=65 outside 0..64"),
        ("a short stride of b", dict(sb=1 - fb), "flow_paste: strides %d (a), %d (b) shorter than the frame's %d bytes" % (fb, 1 - fb, fb)),
        ("short strides of a and out", dict(sa=0, so=0), "flow_paste: strides 0 (a), %d (b) shorter than the frame's %d bytes" % (fb, fb)),
        ("a short stride of out", dict(so=fb - 1), "flow_paste: stride %d (out) shorter than the frame's %d bytes" % (fb - 1, fb)),
        ("short strides of out and mask", dict(so=fb - 1, sm=5), "flow_paste: stride %d (out) shorter than the frame's %d bytes" % (fb - 1, fb)),
        ("a short stride of mask", dict(sm=-767), "flow_paste: stride -767 (mask) shorter than a pair's two planes, 768 bytes"),
        ("a short stride of mask, words at an odd address", dict(sm=767, sbytes=2, a=0x10001, sa=2 * fb, sb=2 * fb, so=2 * fb),
         "flow_paste: stride 767 (mask) shorter than a pair's two planes, 768 bytes"),
        ("words at an odd address", dict(sbytes=2, a=0x10001, sa=2 * fb + 1, sb=2 * fb, so=2 * fb),
         "flow_paste: a payload of 2-byte samples (a, b or out) is not 2-byte aligned"),
        ("words at an odd stride", dict(sbytes=2, sa=2 * fb + 1, sb=2 * fb, so=2 * fb, out=0x20000),
         "flow_paste: strides %d (a), %d (b), %d (out) of 2-byte samples must be even" % (2 * fb + 1, 2 * fb, 2 * fb)),
        ("out overlaps a", dict(out=0x10000 + fb), "flow_paste: out overlaps a, b or mask"),
        ("out overlaps b from below", dict(out=0x20000 - 6 * fb + 1), "flow_paste: out overlaps a, b or mask"),
        ("out overlaps mask", dict(out=0x80000 + 1535), "flow_paste: out overlaps a, b or mask"),
        ("out overlaps mask, counts off", dict(out=0x80000, counts=0x90004), "flow_paste: out overlaps a, b or mask"),
        ("counts off their alignment", dict(counts=0x90004), "flow_paste: counts is not 8-byte aligned"),
    ]
    return ok, rows


def call_entry(args):
    from ssm_amd import hipbind as hb
    lib = hb.load()
    rc = lib.ssm_flow_paste_fwd(args["a"], args["b"], args["sa"], args["sb"], args["out"], args["so"], args["N"], args["T"], args["split"],
                                args["H"], args["W"], args["layout"], args["sbytes"], args["mask"], args["sm"], args["K"], args["counts"], None)
    return rc, lib.ssm_last_error_string().decode()


_OK, _ROWS = entry_cases()
# made-up pointers: host-side refusals only, never on a machine that could launch
no_gpu = pytest.mark.skipif(__import__("torch").cuda.is_available(), reason="made-up pointers: refusals only, never where a launch could follow")


@no_gpu

@pytest.mark.parametrize("name,broken,message", _ROWS, ids=[r[0].replace(" ", "_") for r in _ROWS])
def test_the_entry_refuses_in_order(name, broken, message):
    """Made-up addresses: every case is refused before anything is queued, and the module never sends the valid set itself."""
    assert broken, "a row breaks something"
    assert call_entry(dict(_OK, **broken)) == (-1, message)


@no_gpu
def test_the_entry_refuses_a_frame_of_too_many_strips():
    """2^23 x 2^20 blocks are 2^35 strips; nothing of that size is allocated, the addresses are made up."""
    big = dict(_OK, N=1, T=1, split=0, a=1 << 50, b=1 << 51, out=1 << 52, mask=1 << 53)
    h, w = 8 * (1 << 23), 8 * (1 << 20)
    big.update(H=h, W=w)
    rc, text = call_entry(big)
    assert rc == -1 and text.startswith("flow_paste: a frame of ") and text.endswith("bytes is more than the grid takes")
