"""The flow check's per-block fallback on the GPU: ssm_flow_paste_fwd against flow_paste_host word for word - outputs,
counts and the poisoned bytes around them - in every layout at 8, 10 and 16 bits, and VideoInterpolator(flow_check=True, flow_blocks=K)
against flow_paste_host applied to the outputs of the same run with flow_check=True alone, on masks that flow_consistency_host makes of
the flows FullModel.estimate_flow gives for the same frames.

With the synthetic weights the flows are whatever they are: nothing here reads a count as quality."""
import os
import sys
from fractions import Fraction as Fr

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_hip_flow_check as F  # noqa: E402
import test_hip_video_static as ST  # noqa: E402
import video_cut_clips as C  # noqa: E402
from video_clips import LAYOUTS, V  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SLACK, POISON = 6, 0xA5          # poisoned bytes behind every output row (even: rows of words keep an even pitch)
N, T = 2, 3


# ---- the kernel ---------------------------------------------------------------------------------------------------------------------------
def masks(n, h, w, k, seed):
    """[n, 2, h, w] over {0, 1, 2} at random; in every pair block 0 holds n = k exactly (direction 0 alone) and block 1 n = k + 1
    (direction 1 alone), both among bytes 2."""
    rng = np.random.RandomState(seed + 100 * h + w + k)
    m = rng.randint(0, 3, size=(n, 2, h, w)).astype(np.uint8)
    if (h >> 3) * (w >> 3) >= 2:
        for blk, (d, count) in enumerate(((0, k), (1, min(k + 1, 64)))):
            by, bx = divmod(blk, w >> 3)
            m[:, :, 8 * by:8 * by + 8, 8 * bx:8 * bx + 8] = 2
            flat = np.full(64, 2, np.uint8)
            flat[rng.permutation(64)[:count]] = 1
            m[:, d, 8 * by:8 * by + 8, 8 * bx:8 * bx + 8] = flat.reshape(8, 8)
    return m


def frames_and_outputs(n, t, h, w, layout, bits, seed):
    v = V()
    rng = np.random.RandomState(seed + h + w + layout + bits)
    fb = v.frame_bytes(h, w, layout, bits)
    frames = rng.randint(0, 256, size=(n + 1, fb)).astype(np.uint8)
    wide = np.full((n * t, fb + SLACK), POISON, np.uint8)
    wide[:, :fb] = rng.randint(0, 256, size=(n * t, fb))
    return frames, wide, fb


def check(n, t, h, w, layout, bits, k, split, offset=0, mask_offset=0, seed=0):
    """Kernel == yardstick on pairs (f, f + 1) of one device buffer of n + 1 frames (a and b are rows n, n + 1 of it): outputs with their
    slack, counts with the words around them, the mask inside poisoned slack that stays.  Returns the counts."""
    v = V()
    frames, wide, fb = frames_and_outputs(n, t, h, w, layout, bits, seed)
    m = masks(n, h, w, k, seed)
    want, want_counts = v.flow_paste_host(wide.reshape(n, t, fb + SLACK), frames[:-1], frames[1:], m, h, w, layout, bits, k, split)
    dev, out = ST.device_rows(frames, offset), ST.device_rows(wide, offset)
    mflat = torch.full((mask_offset + m.size + 8,), POISON, dtype=torch.uint8, device=DEV)
    dm = mflat[mask_offset:mask_offset + m.size].view(m.shape)
    dm.copy_(torch.from_numpy(m))
    words = torch.full((n + 2,), -1, dtype=torch.int64, device=DEV)
    v.flow_paste(dev[:-1], dev[1:], out[:, :fb], dm, h, w, layout, bits, k, split, counts=words[1:n + 1])
    torch.cuda.synchronize()
    got, got_counts = out.cpu().numpy(), words.cpu().numpy()
    assert got_counts.tolist() == [-1] + want_counts.tolist() + [-1], (h, w, layout, bits, k, split)
    assert np.array_equal(got, want.reshape(n * t, fb + SLACK)), (h, w, layout, bits, k, split)
    assert np.all(got[:, fb:] == POISON)
    back = mflat.cpu().numpy()
    assert np.array_equal(back[mask_offset:mask_offset + m.size], m.reshape(-1)) and (back[:mask_offset] == POISON).all() \
        and (back[mask_offset + m.size:] == POISON).all(), "the mask is only read"
    assert np.array_equal(dev.cpu().numpy(), frames), "a and b are only read"
    return want_counts


@pytest.mark.parametrize("bits", [8, 10, 16])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_kernel_equals_the_yardstick(layout, bits):
    for h, w in ((16, 24), (17, 23)):
        blocks = V().static_blocks(h, w)
        for k, split in ((20, 0), (31, 1), (0, 3)):
            counts = check(N, T, h, w, layout, bits, k, split)
            assert all(0 < c < blocks for c in counts) or k == 0, "block 0 (n = K) passes, block 1 (n = K + 1) fails"
        assert check(N, T, h, w, layout, bits, 64, 1).tolist() == [0, 0], "K = 64 fails nothing"


@pytest.mark.parametrize("layout, bits", [(0, 8), (3, 10), (2, 16)])
def test_more_than_one_strip(layout, bits):
    """136 x 136: 17 x 17 = 289 blocks, a strip of 256 and a short one; W = 136 keeps every mask row on an 8-byte boundary."""
    counts = check(N, 2, 136, 136, layout, bits, 35, 1, seed=5)
    assert all(50 < c < 239 for c in counts), "random masks, 5 of 9 pixels inconsistent in a direction or the other: n is about 36, K = 35 splits the blocks"


@pytest.mark.parametrize("bits", [8, 16])
def test_operand_bases_off_their_alignment(bits):
    """The payloads' allocation starts 1 byte (bytes) or 2 bytes (words) ahead of them and the mask sits at an odd address: no piece of
    16 x 24 sits on its own boundary.  Then the mask alone off by 4: 8-byte rows that are no 8-byte loads."""
    v = V()
    for layout in (v.CENTRED, v.C422, v.C444):
        check(N, T, 16, 24, layout, bits, 20, 1, offset=v.sample_bytes(bits), mask_offset=1, seed=1)
    check(N, T, 16, 24, v.CENTRED, bits, 20, 2, mask_offset=4, seed=2)


@pytest.mark.parametrize("bits", [8, 10])
def test_negative_strides(bits):
    """a_n = frame N - n, b_n = frame N - n - 1, the masks and the outputs from the last row back: all four strides negative."""
    from ssm_amd import hipbind as hb
    v = V()
    h, w, layout, n, t, k, split = 17, 23, v.C422, 3, 3, 20, 1
    frames, wide, fb = frames_and_outputs(n, t, h, w, layout, bits, seed=2)
    m = masks(n, h, w, k, seed=3)
    want, want_counts = v.flow_paste_host(wide[::-1].reshape(n, t, fb + SLACK), frames[::-1][:-1], frames[::-1][1:], m[::-1], h, w, layout, bits,
                                          k, split)
    dev, out, dm = ST.device_rows(frames), ST.device_rows(wide), torch.from_numpy(m).to(DEV)
    words = torch.full((n + 2,), -1, dtype=torch.int64, device=DEV)
    hb.check(hb.load().ssm_flow_paste_fwd(dev[n].data_ptr(), dev[n - 1].data_ptr(), -dev.stride(0), -dev.stride(0), out[n * t - 1].data_ptr(),
                                          -out.stride(0), n, t, split, h, w, layout, v.sample_bytes(bits), dm[n - 1].data_ptr(), -dm.stride(0), k,
                                          words[1:].data_ptr(), hb.stream_ptr()))
    torch.cuda.synchronize()
    assert words.cpu().numpy().tolist() == [-1] + want_counts.tolist() + [-1]
    assert np.array_equal(out.cpu().numpy()[::-1], want.reshape(n * t, fb + SLACK))
    assert 0 < want_counts[0] < v.static_blocks(h, w)


@pytest.mark.parametrize("bits", [8, 16])
def test_a_frame_without_blocks(bits):
    """7 x 40: the clear alone is queued, the outputs stay untouched."""
    v = V()
    h, w, layout = 7, 40, v.C444
    frames, wide, fb = frames_and_outputs(N, T, h, w, layout, bits, seed=4)
    dev, out = ST.device_rows(frames), ST.device_rows(wide)
    dm = torch.ones(N, 2, h, w, dtype=torch.uint8, device=DEV)
    words = torch.full((N + 2,), -1, dtype=torch.int64, device=DEV)
    v.flow_paste(dev[:-1], dev[1:], out[:, :fb], dm, h, w, layout, bits, 0, 1, counts=words[1:N + 1])
    torch.cuda.synchronize()
    assert words.cpu().numpy().tolist() == [-1, 0, 0, -1] and np.array_equal(out.cpu().numpy(), wide)


# ---- the stream ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    return F.synthetic_model(DEV)


def yardstick_masks(model, payloads, h, w, tag, pairs, pb):
    """{i: mask [2, h, w]} of the pairs by the yardstick, the way test_hip_flow_check.yardstick_checks gets its records: on the flows
    FullModel.estimate_flow gives for the frames as the loop ingests them, `pb` pairs a call (a short last pass filled with its last
    frame)."""
    cfg, m = model
    v, fe = V(), F.FE()
    layout, bits = v.EXTENDED_TAGS[tag]
    planes = v.frames_from_yuv(torch.from_numpy(payloads).to(DEV), h, w, layout, v.default_matrix(h), v.LIMITED, cfg, True, bits=bits)
    top, left = (planes.shape[2] - h) // 2, (planes.shape[3] - w) // 2
    out = {}
    for p0 in range(0, len(pairs), pb):
        group = pairs[p0:p0 + pb]
        sides = [(i, i + 1) for i in group] + [(group[-1] + 1, group[-1] + 1)] * (pb - len(group))
        x = torch.stack([torch.stack([planes[a], planes[b]]) for a, b in sides])
        _, mask = fe.flow_consistency_host(m.estimate_flow(x).cpu().numpy(), top, left, h, w, fe.FLOW_ALPHA, fe.FLOW_BETA)
        out.update({i: mask[p] for p, i in enumerate(group)})
    return out


def repaired(base, payloads, outputs, mask_of, h, w, tag, k, whole=()):
    """flow_paste_host over the outputs `base` of a run without flow_blocks: per pair its outputs in order, split = those below 1/2; the
    pairs in `whole` are left as `base` has them.  -> (the frames, [(i, failed blocks, blocks)] of the pairs that got outputs)."""
    v = V()
    layout, bits = v.EXTENDED_TAGS[tag]
    want, log = base.copy(), []
    for i in sorted({i for i, t in outputs if t > 0}):
        ks = [k_ for k_, (j, t) in enumerate(outputs) if j == i and t > 0]
        split = sum(1 for k_ in ks if outputs[k_][1] < Fr(1, 2))
        res, counts = v.flow_paste_host(base[ks][None], payloads[i:i + 1], payloads[i + 1:i + 2], mask_of[i][None], h, w, layout, bits, k, split)
        if i not in whole:
            want[ks] = res[0]
        log.append((i, int(counts[0]), v.static_blocks(h, w)))
    return want, log


def mixed_k(mask_of, h, w):
    """The largest K that still fails at least one block of the clip, from the measured n of every block."""
    v = V()
    n = np.concatenate([v.flow_block_counts_host(m[None], h, w).reshape(-1) for m in mask_of.values()])
    k = int(n.max()) - 1
    assert k >= 0, "no block of the clip has an inconsistent pixel"
    return k, n


_legs = {}


def leg(model, name):
    if name not in _legs:
        (h, w), n, tag, kw = F.LEGS[name]
        payloads, outputs, plain, report, checks, _ = F.leg(model, name)
        mask_of = yardstick_masks(model, payloads, h, w, tag, list(range(n - 1)), kw["pairs_per_batch"])
        _legs[name] = (payloads, outputs, report, checks, mask_of)
    return _legs[name]


@pytest.mark.parametrize("name", sorted(F.LEGS))
def test_stream_equals_the_yardstick_over_the_plain_run(model, name):
    (h, w), n, tag, kw = F.LEGS[name]
    payloads, outputs, report, checks, mask_of = leg(model, name)
    k, per_block = mixed_k(mask_of, h, w)
    print(name, "K", k, "blocks", per_block.size, "n: least", int(per_block.min()), "largest", int(per_block.max()),
          "failing", int((per_block > k).sum()))
    got, vi = F.stream(model, payloads, h, w, tag, flow_check=True, flow_blocks=k, **kw)
    want, log = repaired(report, payloads, outputs, mask_of, h, w, tag, k)
    assert vi.flow_repaired == log and vi.flow_checks == checks and vi.flow_failed == []
    assert np.array_equal(got, want), int((got != want).sum())
    failed, blocks = sum(f for _, f, _ in log), sum(b for _, _, b in log)
    assert 0 < failed < blocks, "at least one block fails and at least one survives"
    assert not np.array_equal(got, report), "the output differs from the plain run"
    same, vi = F.stream(model, payloads, h, w, tag, flow_check=True, flow_blocks=64, **kw)
    assert np.array_equal(same, report) and vi.flow_repaired == [(i, 0, b) for i, _, b in log], "K = 64: the run with flow_check alone"


def test_with_static_the_static_paste_comes_last(model):
    """The patched clip of the static blocks: the output is static_paste_host(flow_paste_host(plain))."""
    cfg, m = model
    v = V()
    tag, kw = "420jpeg", dict(upsample_rate=3, pairs_per_batch=2)
    clip = ST.patched_clip(tag)
    plain, _ = ST.run(m, cfg, clip, tag, flow_check=True, **kw)
    outputs = [(k_ // 3, Fr(k_ % 3, 3)) for k_ in range((ST.FRAMES - 1) * 3 + 1)]
    mask_of = yardstick_masks(model, clip, ST.H, ST.W, tag, list(range(ST.FRAMES - 1)), 2)
    k, _ = mixed_k(mask_of, ST.H, ST.W)
    mid, log = repaired(plain, clip, outputs, mask_of, ST.H, ST.W, tag, k)
    want, static = ST.pasted(mid, clip, tag, ST.fixed_owner(3))
    got, vi = ST.run(m, cfg, clip, tag, flow_check=True, flow_blocks=k, static=0, **kw)
    assert vi.flow_repaired == log and vi.static == static and all(s == 8 for _, s, _ in static)
    assert np.array_equal(got, want), int((got != want).sum())
    assert sum(f for _, f, _ in log) > 0 and not np.array_equal(got, ST.pasted(plain, clip, tag, ST.fixed_owner(3))[0])


def test_a_cut_pair_and_a_pair_that_reaches_t_are_replaced_whole(model):
    """The scene-cut clip with scene_cut, a T that the worst pairs reach, and flow_blocks: those pairs' outputs are the whole nearer
    frames, the others are pasted per block."""
    h, w = C.SIZES[1]
    payloads = C.cut_clip(h, w)
    tag, kw = "420jpeg", dict(upsample_rate=2, pairs_per_batch=2)
    outputs = F.outputs_of(C.N_FRAMES, kw)
    report, vi0 = F.stream(model, payloads, h, w, tag, flow_check=True, **kw)
    scores = sorted({c.score for _, c in vi0.flow_checks})
    t = scores[-1] if len(scores) > 1 else Fr(2)
    fail = {i for i, c in vi0.flow_checks if c.score >= t}
    whole = fail | {C.CUT}
    mask_of = yardstick_masks(model, payloads, h, w, tag, list(range(C.N_FRAMES - 1)), 2)
    k, _ = mixed_k({i: m_ for i, m_ in mask_of.items() if i not in whole}, h, w)
    got, vi = F.stream(model, payloads, h, w, tag, flow_check=t, scene_cut=C.THRESHOLD, flow_blocks=k, **kw)
    assert [i for i, _ in vi.cuts] == [C.CUT] and {i for i, _ in vi.flow_failed} == fail
    want, log = repaired(F.with_fallback(report, payloads, outputs, whole), payloads, outputs, mask_of, h, w, tag, k, whole=whole)
    assert vi.flow_repaired == log
    assert np.array_equal(got, want), int((got != want).sum())
    assert np.array_equal(got[2 * C.CUT + 1], payloads[C.CUT + 1])
    assert any(f for i, f, _ in log if i not in whole), "a pair that is not replaced whole is pasted per block"


def test_with_the_option_off_nothing_of_it_is_allocated(model):
    v = V()
    clip = v.Clip(64, 96, v.CENTRED, v.BT601, v.LIMITED, model[0], dev=DEV)
    for kw, lead in ((dict(), 0), (dict(flow_check=(None, 0.01, 0.5)), 0), (dict(scene_cut=Fr(1, 10)), 1), (dict(static=0), 1)):
        opt = v.PairOptions(None, clip, **kw)
        opt.buffers(2, 4, 2, 2, 4)
        assert opt.lead == lead and opt.dev_mask is None and not hasattr(opt, "dev_failed"), kw
    opt = v.PairOptions(None, clip, flow_check=(None, 0.01, 0.5), flow_blocks=5)
    opt.buffers(2, 4, 2, 2, 4)
    assert opt.lead == 1 and [tuple(m_.shape) for m_ in opt.dev_mask] == [(2, 2, 64, 96)] * 2
