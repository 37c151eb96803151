"""Blocks that do not change on the GPU: ssm_static_paste_fwd against static_paste_host word for word - outputs, counts and
the poisoned bytes around them - in every layout at 8, 10 and 16 bits, and VideoInterpolator(static=0) against static_paste_host applied
to the outputs of the same run without the option.

The frames of a kernel test are built pair by pair (make_frames): frame f + 1 is random, then about half of its blocks are frame f's, one
block sits exactly at d = lo (split between a luma and a U sample), one at d = lo + 1 (a V sample), one differs in a single V sample by 1
and one is equal in luma and V and different in every U sample."""
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import field_clips  # noqa: E402
from video_clips import LAYOUTS, V, frames_of, synthetic_model, y4m  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SIZES = ((24, 40), (27, 45))          # every sample in a block; trailing rows and columns, odd chroma sizes, planes that start anywhere
SLACK = 6                              # poisoned bytes behind every output row (even: rows of words keep an even pitch)
POISON = 0xA5


def chroma_block(layout):
    v = V()
    return (8, 8) if layout == v.C444 else (8, 4) if layout == v.C422 else (4, 4)


def make_frames(h, w, layout, bits, count, lo, seed=0):
    """[count, frame_bytes] uint8: see the module's docstring; every pair (f, f + 1) has the five kinds of block."""
    v = V()
    rng = np.random.RandomState(seed + 1000 * h + 10 * w + layout + bits + 7 * lo)
    fb, top = v.frame_bytes(h, w, layout, bits), (1 << bits) - 1
    buf = rng.randint(0, 256, size=(count, fb)).astype(np.uint8)
    if bits > 8:
        buf.view("<u2")[...] &= top
    y, u, c = v.split_planes(buf, h, w, layout, bits)          # views of buf
    cr, cc = chroma_block(layout)
    blocks = [(by, bx) for by in range(h >> 3) for bx in range(w >> 3)]
    assert len(blocks) >= 6

    def step(plane, f, row, col, by):          # sample (row, col) of frame f + 1 = frame f's, moved by `by` inside the depth
        s = int(plane[f, row, col])
        plane[f + 1, row, col] = s + by if s + by <= top else s - by

    for f in range(count - 1):
        for k, (by, bx) in enumerate(blocks):
            if k % 2 == 0 or k < 5:
                for p, (rr, rc) in ((y, (8, 8)), (u, (cr, cc)), (c, (cr, cc))):
                    p[f + 1, rr * by:rr * by + rr, rc * bx:rc * bx + rc] = p[f, rr * by:rr * by + rr, rc * bx:rc * bx + rc]
        (y0, x0), (y1, x1), (y2, x2), (y3, x3) = blocks[1:5]
        if lo:                                                       # block 1: d = lo exactly
            step(y, f, 8 * y0 + 7, 8 * x0 + 7, lo - lo // 2)
            step(u, f, cr * y0, cc * x0 + cc - 1, lo // 2)
        step(c, f, cr * y1 + cr - 1, cc * x1, lo + 1)                # block 2: d = lo + 1
        step(c, f, cr * y2, cc * x2, 1)                              # block 3: a single V sample, by 1
        u[f + 1, cr * y3:cr * y3 + cr, cc * x3:cc * x3 + cc] ^= 1 << (bits - 1)          # block 4: U alone, every sample
    return buf


def device_rows(host, offset=0):
    """The rows of `host` [R, bytes] on the device, in one allocation that starts `offset` bytes before them."""
    flat = torch.empty(offset + host.size, dtype=torch.uint8, device=DEV)
    rows = flat[offset:].view(host.shape)
    rows.copy_(torch.from_numpy(host))
    return rows


def poisoned_outputs(n, t, fb, seed):
    rng = np.random.RandomState(seed)
    wide = np.full((n * t, fb + SLACK), POISON, np.uint8)
    wide[:, :fb] = rng.randint(0, 256, size=(n * t, fb))
    return wide


def check(frames, n, t, h, w, layout, bits, lo, offset=0):
    """Kernel == yardstick on pairs (f, f + 1) of `frames` as two views of one device buffer of n + 1 frames: outputs with their slack,
    counts with the words around them.  Returns the counts."""
    v = V()
    fb = v.frame_bytes(h, w, layout, bits)
    assert frames.shape == (n + 1, fb)
    dev = device_rows(frames, offset)
    wide = poisoned_outputs(n, t, fb, seed=n + 10 * t)
    want, want_counts = v.static_paste_host(wide.reshape(n, t, fb + SLACK), frames[:-1], frames[1:], h, w, layout, bits, lo)
    out = device_rows(wide, offset)
    words = torch.full((n + 2,), -1, dtype=torch.int64, device=DEV)
    v.static_paste(dev[:-1], dev[1:], out[:, :fb], h, w, layout, bits, lo, counts=words[1:n + 1])
    torch.cuda.synchronize()
    got, got_counts = out.cpu().numpy(), words.cpu().numpy()
    assert got_counts[0] == -1 and got_counts[-1] == -1, "the words around counts stay"
    assert got_counts[1:n + 1].tolist() == want_counts.tolist(), (h, w, layout, bits, lo, n, t)
    assert np.array_equal(got, want.reshape(n * t, fb + SLACK)), (h, w, layout, bits, lo, n, t)
    assert np.all(got[:, fb:] == POISON)
    return want_counts


@pytest.mark.parametrize("bits", [8, 10, 16])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_kernel_equals_the_yardstick(layout, bits):
    for h, w in SIZES:
        blocks = V().static_blocks(h, w)
        for lo in (0, 37):
            frames = make_frames(h, w, layout, bits, 4, lo)
            for n in (1, 3):
                for t in (1, 3):
                    counts = check(frames[:n + 1], n, t, h, w, layout, bits, lo)
                    # blocks 0, 6, 8, .. are frame f's; block 1 (d = lo) always, block 3 (d = 1) with lo = 37; blocks 2 and 4 never
                    assert counts.tolist() == [len(range(0, blocks, 2)) - 2 + 1 + (1 if lo else 0)] * n
                    assert blocks // 3 < counts[0] < 2 * blocks // 3, "about half"


@pytest.mark.parametrize("layout, bits", [(0, 8), (3, 10), (2, 16)])
def test_more_than_one_workgroup(layout, bits):
    """136 x 268: 17 x 33 = 561 blocks, three strips of 256 with the last one short, rows of blocks that cross from strip to strip; W is
    no multiple of 8, so in 4:2:0 and 4:2:2 every other chroma row starts off its piece's boundary."""
    h, w = 136, 268
    frames = make_frames(h, w, layout, bits, 3, 37, seed=5)
    counts = check(frames, 2, 2, h, w, layout, bits, 37)
    assert counts.tolist() == [len(range(0, 561, 2))] * 2, "the even blocks less blocks 2 and 4, and blocks 1 and 3"


@pytest.mark.parametrize("bits", [8, 16])
def test_operand_bases_off_their_alignment(bits):
    """The operands' allocation starts 1 byte (bytes) or 2 bytes (words) ahead of them: no piece of 24 x 40 sits on its own boundary."""
    v = V()
    for layout in (v.CENTRED, v.C422, v.C444):
        frames = make_frames(24, 40, layout, bits, 4, 37, seed=1)
        check(frames, 3, 3, 24, 40, layout, bits, 37, offset=v.sample_bytes(bits))


@pytest.mark.parametrize("bits", [8, 10])
def test_negative_strides(bits):
    """a_n = frame N - n, b_n = frame N - n - 1 and the outputs from the last row back: all three strides negative."""
    from ssm_amd import hipbind as hb
    v = V()
    h, w, layout, n, t, lo = 27, 45, v.C422, 3, 3, 37
    fb = v.frame_bytes(h, w, layout, bits)
    frames = make_frames(h, w, layout, bits, n + 1, lo, seed=2)
    wide = poisoned_outputs(n, t, fb, seed=4)
    want, want_counts = v.static_paste_host(wide[::-1].reshape(n, t, fb + SLACK), frames[::-1][:-1], frames[::-1][1:], h, w, layout, bits, lo)
    dev, out = device_rows(frames), device_rows(wide)
    words = torch.full((n + 2,), -1, dtype=torch.int64, device=DEV)
    hb.check(hb.load().ssm_static_paste_fwd(dev[n].data_ptr(), dev[n - 1].data_ptr(), -dev.stride(0), -dev.stride(0), out[n * t - 1].data_ptr(),
                                            -out.stride(0), n, t, h, w, layout, v.sample_bytes(bits), lo, words[1:].data_ptr(), hb.stream_ptr()))
    torch.cuda.synchronize()
    assert words.cpu().numpy().tolist() == [-1] + want_counts.tolist() + [-1]
    assert np.array_equal(out.cpu().numpy()[::-1], want.reshape(n * t, fb + SLACK))
    assert 0 < want_counts[0] < v.static_blocks(h, w)


@pytest.mark.parametrize("bits", [8, 16])
def test_degenerate_frames(bits):
    v = V()
    # no block: outputs as they were, counts cleared
    h, w, layout = 7, 64, v.C444
    fb = v.frame_bytes(h, w, layout, bits)
    frames = np.random.RandomState(bits).randint(0, 256, size=(3, fb)).astype(np.uint8)
    frames[1] = frames[0]
    wide = poisoned_outputs(2, 2, fb, seed=1)
    dev, out = device_rows(frames), device_rows(wide)
    words = torch.full((4,), -1, dtype=torch.int64, device=DEV)
    v.static_paste(dev[:-1], dev[1:], out[:, :fb], h, w, layout, bits, 0, counts=words[1:3])
    torch.cuda.synchronize()
    assert words.cpu().numpy().tolist() == [-1, 0, 0, -1] and np.array_equal(out.cpu().numpy(), wide)
    # a equal to b: every block static, the trailing samples keep their bytes
    for layout in (v.CENTRED, v.C422):
        h, w = 27, 45
        fb = v.frame_bytes(h, w, layout, bits)
        frames = np.repeat(np.random.RandomState(bits + layout).randint(0, 256, size=(1, fb)).astype(np.uint8), 3, axis=0)
        counts = check(frames, 2, 2, h, w, layout, bits, 0)
        assert counts.tolist() == [15, 15]
        wide = poisoned_outputs(2, 2, fb, seed=12)
        got, _ = v.static_paste_host(wide.reshape(2, 2, fb + SLACK), frames[:-1], frames[1:], h, w, layout, bits, 0)
        planes = (v.split_planes(np.ascontiguousarray(x[:, :fb]), h, w, layout, bits) for x in (got.reshape(4, -1), wide, np.repeat(frames[:1], 4, axis=0)))
        cr, cc = chroma_block(layout)
        for (g, o, a), (rr, rc) in zip(zip(*planes), ((8, 8), (cr, cc), (cr, cc))):
            rows, cols = 3 * rr, 5 * rc          # 3 x 5 blocks
            assert np.array_equal(g[:, :rows, :cols], a[:, :rows, :cols])
            assert np.array_equal(g[:, rows:], o[:, rows:]) and np.array_equal(g[:, :, cols:], o[:, :, cols:])
            assert g.shape[1] > rows and g.shape[2] > cols, "every plane has trailing samples"


# ---- the stream ----------------------------------------------------------------------------------------------------------------------------
H, W, FRAMES = 64, 96, 6


@pytest.fixture(scope="module")
def model():
    return synthetic_model(DEV)


def patched_clip(tag, patches=True, speed=1.0):
    """The moving texture of tests/field_clips.py with a block-aligned 16 x 24 patch of constant samples at (8, 16) and a second one at
    (35, 53): of that only the blocks it covers whole - block row 5, block columns 7 and 8 - are the same in every frame."""
    v = V()
    layout, bits = v.EXTENDED_TAGS[tag]
    clip = field_clips.payloads("progressive", FRAMES, H, W, tag, v=speed)
    if patches:
        y = v.split_planes(clip, H, W, layout, bits)[0]
        y[:, 8:24, 16:40] = 90 << (bits - 8)
        y[:, 35:51, 53:77] = 170 << (bits - 8)
    return clip


def run(m, cfg, clip, tag, **kw):
    """The clip through VideoInterpolator(**kw): (the frames written, the interpolator)."""
    v = V()
    r = v.Y4MReader(y4m(clip, H, W, tag), extended=True)
    sink = io.BytesIO()
    wr = v.Y4MWriter.like(sink, r)
    vi = v.VideoInterpolator(m, cfg, **kw)
    count = vi.run(r, wr)
    assert count == wr.frames_written
    return frames_of(sink.getvalue()), vi


def pasted(plain, clip, tag, owner):
    """static_paste_host at lo = 0 over the outputs `plain` of a run without the option: owner[k] = the pair i of output k, or None for an
    output that is an input frame.  -> (the frames, [(i, static blocks, blocks)] of the pairs that got outputs)."""
    v = V()
    layout, bits = v.EXTENDED_TAGS[tag]
    want, static = plain.copy(), []
    for i in sorted(set(o for o in owner if o is not None)):
        ks = [k for k, o in enumerate(owner) if o == i]
        res, counts = v.static_paste_host(plain[ks][None], clip[i:i + 1], clip[i + 1:i + 2], H, W, layout, bits, 0)
        want[ks] = res[0]
        static.append((i, int(counts[0]), v.static_blocks(H, W)))
    return want, static


def fixed_owner(rate):
    return [None if k % rate == 0 else k // rate for k in range((FRAMES - 1) * rate + 1)]


@pytest.mark.parametrize("tag", ["420jpeg", "422p10"])
@pytest.mark.parametrize("kw", [dict(upsample_rate=2), dict(upsample_rate=3), dict(upsample_rate=3, pairs_per_batch=2),
                                dict(upsample_rate=2, flow_scale=2)], ids=["x2", "x3", "x3-pb2", "x2-coarse"])
def test_fixed_grid_keeps_the_static_blocks(model, tag, kw):
    cfg, m = model
    clip = patched_clip(tag)
    plain, _ = run(m, cfg, clip, tag, **kw)
    got, vi = run(m, cfg, clip, tag, static=0, **kw)
    want, static = pasted(plain, clip, tag, fixed_owner(kw["upsample_rate"]))
    assert vi.static == static and [s for _, s, _ in static] == [8] * (FRAMES - 1), "2 x 3 blocks of the first patch, 1 x 2 of the second"
    assert np.array_equal(got, want)
    assert not np.array_equal(got, plain), "the synthesised patch differs from the input's somewhere: the option does something"


@pytest.mark.parametrize("tag", ["420jpeg", "422p10"])
@pytest.mark.parametrize("pb", [1, 2])
def test_timeline_keeps_the_static_blocks(model, tag, pb):
    """240 -> 640 frames/s: step 3/8, pairs with two and with three outputs; of the input frames only 0 and 3 are written."""
    cfg, m = model
    v = V()
    clip = patched_clip(tag)
    kw = dict(target_rate=(640, 1), pairs_per_batch=pb)          # the clips of y4m() run at 240 frames/s
    plain, ref = run(m, cfg, clip, tag, **kw)
    got, vi = run(m, cfg, clip, tag, static=0, **kw)
    tl = ref.timeline((240, 1))
    owner = []
    for k in range(plain.shape[0]):
        i, t = tl.at(k)
        owner.append(i if t else None)
    assert sorted(set(len([o for o in owner if o == i]) for i in range(FRAMES - 1))) == [2, 3]
    want, static = pasted(plain, clip, tag, owner)
    assert vi.static == static and all(s == 8 for _, s, _ in static)
    assert np.array_equal(got, want) and not np.array_equal(got, plain)


def test_scene_cut_replaces_a_cut_pairs_frames_whole(model):
    """Frames 3.. are the clip negated: pair (2, 3) is a cut, its outputs are the run-with-scene_cut's (input frames, whole); the other pairs
    keep their static blocks.  The patches are negated too, so the cut pair has no static block."""
    cfg, m = model
    tag = "420jpeg"
    clip = patched_clip(tag, speed=0.25)          # slow motion: the score of an ordinary pair stays far below the cut's
    clip[3:] = 255 - clip[3:]
    kw = dict(upsample_rate=3, scene_cut="1/10", pairs_per_batch=2)
    plain, ref = run(m, cfg, clip, tag, **kw)
    got, vi = run(m, cfg, clip, tag, static=0, **kw)
    assert [i for i, _ in ref.cuts] == [2] and vi.cuts == ref.cuts
    want, static = pasted(plain, clip, tag, fixed_owner(3))
    assert vi.static == static and [s for _, s, _ in static] == [8, 8, 0, 8, 8]
    assert np.array_equal(got, want)
    assert np.array_equal(got[7], clip[2]) and np.array_equal(got[8], clip[3])


def test_a_clip_without_an_equal_block_comes_out_as_it_does_without_the_option(model):
    cfg, m = model
    clip = patched_clip("420jpeg", patches=False)
    clip[:, H * W:] = np.random.RandomState(3).randint(16, 240, size=clip[:, H * W:].shape)          # chroma that differs from frame to frame
    plain, _ = run(m, cfg, clip, "420jpeg", upsample_rate=2)
    got, vi = run(m, cfg, clip, "420jpeg", upsample_rate=2, static=0)
    assert vi.static == [(i, 0, 96) for i in range(FRAMES - 1)]
    assert np.array_equal(got, plain)
