"""The per-block fallback as a cross-fade on the GPU: ssm_flow_mix_fwd against flow_mix_host word for word - outputs, counts
and the poisoned bytes around them - in every layout at 8, 10 and 16 bits, its two ends against ssm_flow_paste_fwd on the device, and
VideoInterpolator(flow_check=True, flow_blocks=63, flow_fallback="mix") against flow_mix_host applied to the outputs of the same run with
flow_check=True alone, on the masks and the legs of test_hip_flow_repair.

With the synthetic weights the flows are whatever they are: nothing here reads a count, or a mixed block, as quality."""
import os
import sys
from fractions import Fraction as Fr

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_hip_flow_check as F  # noqa: E402
import test_hip_flow_repair as P  # noqa: E402
import test_hip_video_static as ST  # noqa: E402
import video_cut_clips as C  # noqa: E402
from video_clips import LAYOUTS, V  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = P.DEV
SLACK, POISON = P.SLACK, P.POISON
N, T = 2, 3
K_STREAM = 63          # the K of the stream tests: a block fails iff all 64 of its pixels are inconsistent


# ---- the kernel ---------------------------------------------------------------------------------------------------------------------------
def extreme_frames(frames, seed):
    """The same payloads with every 16-bit word one of 0, 1, 65534, 65535: with den = 65535 the numerators reach 65535 * 65535 + 32767."""
    rng = np.random.RandomState(seed)
    words = np.array([0, 1, 65534, 65535], "<u2")[rng.randint(0, 4, size=frames.size // 2)]
    return words.view(np.uint8).reshape(frames.shape)


def check(n, t, h, w, layout, bits, k, mix, offset=0, mask_offset=0, seed=0, extreme=False):
    """Kernel == yardstick on pairs (f, f + 1) of one device buffer of n + 1 frames (a and b are rows n, n + 1 of it) with
    mix = (num0, num_step, den): outputs with their slack, counts with the words around them, the mask inside poisoned slack that
    stays.  Returns the counts."""
    v = V()
    frames, wide, fb = P.frames_and_outputs(n, t, h, w, layout, bits, seed)
    if extreme:
        frames = extreme_frames(frames, seed)
    m = P.masks(n, h, w, k, seed)
    want, want_counts = v.flow_mix_host(wide.reshape(n, t, fb + SLACK), frames[:-1], frames[1:], m, h, w, layout, bits, k, *mix)
    dev, out = ST.device_rows(frames, offset), ST.device_rows(wide, offset)
    mflat = torch.full((mask_offset + m.size + 8,), POISON, dtype=torch.uint8, device=DEV)
    dm = mflat[mask_offset:mask_offset + m.size].view(m.shape)
    dm.copy_(torch.from_numpy(m))
    words = torch.full((n + 2,), -1, dtype=torch.int64, device=DEV)
    v.flow_mix(dev[:-1], dev[1:], out[:, :fb], dm, h, w, layout, bits, k, *mix, counts=words[1:n + 1])
    torch.cuda.synchronize()
    got, got_counts = out.cpu().numpy(), words.cpu().numpy()
    assert got_counts.tolist() == [-1] + want_counts.tolist() + [-1], (h, w, layout, bits, k, mix)
    assert np.array_equal(got, want.reshape(n * t, fb + SLACK)), (h, w, layout, bits, k, mix, int((got != want.reshape(got.shape)).sum()))
    assert np.all(got[:, fb:] == POISON)
    back = mflat.cpu().numpy()
    assert np.array_equal(back[mask_offset:mask_offset + m.size], m.reshape(-1)) and (back[:mask_offset] == POISON).all() \
        and (back[mask_offset + m.size:] == POISON).all(), "the mask is only read"
    assert np.array_equal(dev.cpu().numpy(), frames), "a and b are only read"
    if want_counts.sum():
        assert not np.array_equal(want.reshape(n * t, fb + SLACK), wide), "a failed block changes"
    return want_counts


@pytest.mark.parametrize("bits", [8, 10, 16])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_kernel_equals_the_yardstick(layout, bits):
    """T = 3: the fixed grid of rate 8's first outputs, thirds up to t = 1, and 0, 1/2, 1 over 1000."""
    for h, w in ((16, 24), (17, 23)):
        blocks = V().static_blocks(h, w)
        for k, mix in ((20, (1, 1, 8)), (31, (1, 1, 3)), (0, (0, 500, 1000)), (20, (3, -1, 5))):
            counts = check(N, T, h, w, layout, bits, k, mix)
            assert all(0 < c < blocks for c in counts) or k == 0, "block 0 (n = K) passes, block 1 (n = K + 1) fails"
        assert check(N, T, h, w, layout, bits, 64, (1, 1, 4)).tolist() == [0, 0], "K = 64 fails nothing"


@pytest.mark.parametrize("layout, bits", [(0, 8), (3, 10), (2, 16)])
def test_more_than_one_strip(layout, bits):
    """136 x 136: 17 x 17 = 289 blocks, a strip of 256 and a short one; W = 136 keeps every mask row on an 8-byte boundary."""
    counts = check(N, 2, 136, 136, layout, bits, 35, (2, 2, 5), seed=5)
    assert all(50 < c < 239 for c in counts), "random masks, 5 of 9 pixels inconsistent in a direction or the other: n is about 36, K = 35 splits the blocks"


@pytest.mark.parametrize("bits", [8, 16])
def test_operand_bases_off_their_alignment(bits):
    """The payloads' allocation starts 1 byte (bytes) or 2 bytes (words) ahead of them and the mask sits at an odd address: no piece of
    16 x 24 sits on its own boundary.  Then the mask alone off by 4: 8-byte rows that are no 8-byte loads."""
    v = V()
    for layout in (v.CENTRED, v.C422, v.C444):
        check(N, T, 16, 24, layout, bits, 20, (1, 1, 4), offset=v.sample_bytes(bits), mask_offset=1, seed=1)
    check(N, T, 16, 24, v.CENTRED, bits, 20, (1, 1, 4), mask_offset=4, seed=2)


@pytest.mark.parametrize("bits", [8, 10])
def test_negative_strides(bits):
    """a_n = frame N - n, b_n = frame N - n - 1 - rows of one buffer - the masks and the outputs from the last row back: all four strides
    negative."""
    from ssm_amd import hipbind as hb
    v = V()
    h, w, layout, n, t, k, mix = 17, 23, v.C422, 3, 3, 20, (1, 2, 7)
    frames, wide, fb = P.frames_and_outputs(n, t, h, w, layout, bits, seed=2)
    m = P.masks(n, h, w, k, seed=3)
    want, want_counts = v.flow_mix_host(wide[::-1].reshape(n, t, fb + SLACK), frames[::-1][:-1], frames[::-1][1:], m[::-1], h, w, layout, bits,
                                        k, *mix)
    dev, out, dm = ST.device_rows(frames), ST.device_rows(wide), torch.from_numpy(m).to(DEV)
    words = torch.full((n + 2,), -1, dtype=torch.int64, device=DEV)
    hb.check(hb.load().ssm_flow_mix_fwd(dev[n].data_ptr(), dev[n - 1].data_ptr(), -dev.stride(0), -dev.stride(0), out[n * t - 1].data_ptr(),
                                        -out.stride(0), n, t, *mix, h, w, layout, v.sample_bytes(bits), dm[n - 1].data_ptr(), -dm.stride(0), k,
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
    frames, wide, fb = P.frames_and_outputs(N, T, h, w, layout, bits, seed=4)
    dev, out = ST.device_rows(frames), ST.device_rows(wide)
    dm = torch.ones(N, 2, h, w, dtype=torch.uint8, device=DEV)
    words = torch.full((N + 2,), -1, dtype=torch.int64, device=DEV)
    v.flow_mix(dev[:-1], dev[1:], out[:, :fb], dm, h, w, layout, bits, 0, 1, 1, 4, counts=words[1:N + 1])
    torch.cuda.synchronize()
    assert words.cpu().numpy().tolist() == [-1, 0, 0, -1] and np.array_equal(out.cpu().numpy(), wide)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_the_largest_numerator(layout):
    """den = 65535 on words that are 0, 1, 65534 or 65535, at k = 1 and k = 65534: 65535 * 65534 + 65535 + 32767 and its neighbours."""
    counts = check(N, 2, 17, 23, layout, 16, 0, (1, 65533, 65535), seed=6, extreme=True)
    assert counts.sum() > 0
    check(N, 2, 16, 24, layout, 16, 20, (65535, -65535, 65535), seed=7, extreme=True)


@pytest.mark.parametrize("bits", [8, 10, 16])
def test_den_1001_and_a_single_output(bits):
    """29.97 -> 25 frames/s: the times 77/1001 + j 308/1001; then T = 1 with num_step = 0, with N = 2 and with N T = 1, whose strides
    name nothing."""
    v = V()
    check(N, 4, 17, 23, v.C422, bits, 20, (77, 308, 1001), seed=8)
    check(N, 1, 16, 24, v.CENTRED, bits, 20, (400, 0, 1000), seed=9)
    check(1, 1, 17, 23, v.C444, bits, 0, (1, 0, 2), seed=10)


@pytest.mark.parametrize("layout, bits", [(0, 8), (1, 16), (2, 10), (3, 16)])
def test_the_ends_are_the_nearer_kernel_on_the_device(layout, bits):
    """k_j = 0 writes what ssm_flow_paste_fwd writes with split = T, k_j = den what it writes with split = 0: outputs and counts."""
    v = V()
    h, w, k = 17, 23, 20
    frames, wide, fb = P.frames_and_outputs(N, T, h, w, layout, bits, seed=11)
    dev, dm = ST.device_rows(frames), torch.from_numpy(P.masks(N, h, w, k, seed=11)).to(DEV)
    for den in (2, 1001, 65535):
        for num0, split in ((0, T), (den, 0)):
            out_mix, out_paste = ST.device_rows(wide), ST.device_rows(wide)
            c_mix = v.flow_mix(dev[:-1], dev[1:], out_mix[:, :fb], dm, h, w, layout, bits, k, num0, 0, den)
            c_paste = v.flow_paste(dev[:-1], dev[1:], out_paste[:, :fb], dm, h, w, layout, bits, k, split)
            torch.cuda.synchronize()
            assert torch.equal(out_mix, out_paste) and torch.equal(c_mix, c_paste) and int(c_mix.sum()) > 0, (den, num0)
            assert not np.array_equal(out_mix.cpu().numpy(), wide)


# ---- the stream ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    return F.synthetic_model(DEV)


def den_of(kw):
    """The den of a leg: upsample_rate on the fixed grid, the denominator of the timeline's step otherwise."""
    v = V()
    return v.Timeline(v.timeline_step(F.IN_RATE, kw["target_rate"])).step.denominator if "target_rate" in kw else kw["upsample_rate"]


def mixed(base, payloads, outputs, mask_of, h, w, tag, k, den, whole=()):
    """flow_mix_host over the outputs `base` of a run without flow_blocks: per pair its outputs in order, their exact times as whole
    numbers over den; the pairs in `whole` are left as `base` has them.  -> (the frames, [(i, failed blocks, blocks)] of the pairs that
    got outputs)."""
    v = V()
    layout, bits = v.EXTENDED_TAGS[tag]
    want, log = base.copy(), []
    for i in sorted({i for i, t in outputs if t > 0}):
        rows = [k_ for k_, (j, t) in enumerate(outputs) if j == i and t > 0]
        ks = [outputs[k_][1] * den for k_ in rows]
        assert all(x.denominator == 1 for x in ks)
        num0, step = int(ks[0]), int(ks[1] - ks[0]) if len(ks) > 1 else 0
        assert [num0 + j * step for j in range(len(ks))] == ks
        res, counts = v.flow_mix_host(base[rows][None], payloads[i:i + 1], payloads[i + 1:i + 2], mask_of[i][None], h, w, layout, bits, k, num0,
                                      step, den)
        if i not in whole:
            want[rows] = res[0]
        log.append((i, int(counts[0]), v.static_blocks(h, w)))
    return want, log


@pytest.mark.parametrize("name", sorted(F.LEGS))
def test_stream_equals_the_yardstick_over_the_plain_run(model, name):
    (h, w), n, tag, kw = F.LEGS[name]
    payloads, outputs, report, checks, mask_of = P.leg(model, name)
    got, vi = F.stream(model, payloads, h, w, tag, flow_check=True, flow_blocks=K_STREAM, flow_fallback="mix", **kw)
    want, log = mixed(report, payloads, outputs, mask_of, h, w, tag, K_STREAM, den_of(kw))
    failed, blocks = sum(f for _, f, _ in log), sum(b for _, _, b in log)
    print(name, "K", K_STREAM, "den", den_of(kw), "blocks", blocks, "failing", failed, "bytes that differ from the plain run",
          int((want != report).sum()))
    assert vi.flow_repaired == log and vi.flow_checks == checks and vi.flow_failed == []
    assert np.array_equal(got, want), int((got != want).sum())
    assert 0 < failed < blocks, "at least one block fails and at least one survives"
    near, vi_near = F.stream(model, payloads, h, w, tag, flow_check=True, flow_blocks=K_STREAM, flow_fallback="nearer", **kw)
    want_near, log_near = P.repaired(report, payloads, outputs, mask_of, h, w, tag, K_STREAM)
    assert np.array_equal(near, want_near) and vi_near.flow_repaired == log_near == log, "nearer: the run with flow_blocks alone"
    assert not np.array_equal(got, near), "both runs differ from the plain one in failed blocks alone: a failed block differs between them"
    same, vi = F.stream(model, payloads, h, w, tag, flow_check=True, flow_blocks=64, flow_fallback="mix", **kw)
    assert np.array_equal(same, report) and vi.flow_repaired == [(i, 0, b) for i, _, b in log], "K = 64: the run with flow_check alone"


def test_nearer_is_the_run_without_the_option_byte_for_byte(model):
    name = "rate3_pb2"
    (h, w), n, tag, kw = F.LEGS[name]
    payloads = P.leg(model, name)[0]
    plain, vi0 = F.stream(model, payloads, h, w, tag, flow_check=True, flow_blocks=K_STREAM, **kw)
    near, vi1 = F.stream(model, payloads, h, w, tag, flow_check=True, flow_blocks=K_STREAM, flow_fallback="nearer", **kw)
    assert np.array_equal(plain, near) and vi0.flow_repaired == vi1.flow_repaired and vi0.flow_checks == vi1.flow_checks


def test_with_static_the_static_paste_comes_last(model):
    """The patched clip of the static blocks: the output is static_paste_host(flow_mix_host(plain)), the static blocks the left frame's."""
    cfg, m = model
    tag, kw = "420jpeg", dict(upsample_rate=3, pairs_per_batch=2)
    clip = ST.patched_clip(tag)
    plain, _ = ST.run(m, cfg, clip, tag, flow_check=True, **kw)
    outputs = [(k_ // 3, Fr(k_ % 3, 3)) for k_ in range((ST.FRAMES - 1) * 3 + 1)]
    mask_of = P.yardstick_masks(model, clip, ST.H, ST.W, tag, list(range(ST.FRAMES - 1)), 2)
    k, _ = P.mixed_k(mask_of, ST.H, ST.W)
    mid, log = mixed(plain, clip, outputs, mask_of, ST.H, ST.W, tag, k, 3)
    want, static = ST.pasted(mid, clip, tag, ST.fixed_owner(3))
    got, vi = ST.run(m, cfg, clip, tag, flow_check=True, flow_blocks=k, flow_fallback="mix", static=0, **kw)
    assert vi.flow_repaired == log and vi.static == static and all(s == 8 for _, s, _ in static)
    assert np.array_equal(got, want), int((got != want).sum())
    assert sum(f for _, f, _ in log) > 0 and not np.array_equal(got, ST.pasted(plain, clip, tag, ST.fixed_owner(3))[0])


def test_a_cut_pair_and_a_pair_that_reaches_t_are_replaced_whole_by_the_nearer_frame(model):
    """The scene-cut clip with scene_cut, a T that the worst pairs reach, flow_blocks and mix: those pairs' outputs are the whole NEARER
    frames - no cross-fade across a cut - the others are mixed per block."""
    h, w = C.SIZES[1]
    payloads = C.cut_clip(h, w)
    tag, kw = "420jpeg", dict(upsample_rate=2, pairs_per_batch=2)
    outputs = F.outputs_of(C.N_FRAMES, kw)
    report, vi0 = F.stream(model, payloads, h, w, tag, flow_check=True, **kw)
    scores = sorted({c.score for _, c in vi0.flow_checks})
    t = scores[-1] if len(scores) > 1 else Fr(2)
    fail = {i for i, c in vi0.flow_checks if c.score >= t}
    whole = fail | {C.CUT}
    mask_of = P.yardstick_masks(model, payloads, h, w, tag, list(range(C.N_FRAMES - 1)), 2)
    k, _ = P.mixed_k({i: m_ for i, m_ in mask_of.items() if i not in whole}, h, w)
    got, vi = F.stream(model, payloads, h, w, tag, flow_check=t, scene_cut=C.THRESHOLD, flow_blocks=k, flow_fallback="mix", **kw)
    assert [i for i, _ in vi.cuts] == [C.CUT] and {i for i, _ in vi.flow_failed} == fail
    want, log = mixed(F.with_fallback(report, payloads, outputs, whole), payloads, outputs, mask_of, h, w, tag, k, 2, whole=whole)
    assert vi.flow_repaired == log
    assert np.array_equal(got, want), int((got != want).sum())
    assert np.array_equal(got[2 * C.CUT + 1], payloads[C.CUT + 1]), "t = 1/2 of a cut pair: the right frame, whole"
    assert any(f for i, f, _ in log if i not in whole), "a pair that is not replaced whole is mixed per block"


def test_with_the_option_off_nothing_of_it_is_allocated(model):
    """mix launches another kernel on flow_blocks' own operands: the buffers are those of nearer, and without flow_blocks there are none."""
    v = V()
    clip = v.Clip(64, 96, v.CENTRED, v.BT601, v.LIMITED, model[0], dev=DEV)
    for kw in (dict(), dict(flow_check=(None, 0.01, 0.5)), dict(flow_check=(None, 0.01, 0.5), flow_fallback="nearer")):
        opt = v.PairOptions(None, clip, **kw)
        opt.buffers(2, 4, 2, 2, 4)
        assert opt.lead == 0 and opt.dev_mask is None and not hasattr(opt, "dev_failed") and not opt.flow_mix, kw
    held = []
    for fallback in ("nearer", "mix"):
        opt = v.PairOptions(None, clip, flow_check=(None, 0.01, 0.5), flow_blocks=5, flow_fallback=fallback)
        opt.buffers(2, 4, 2, 2, 4)
        assert opt.lead == 1 and [tuple(m_.shape) for m_ in opt.dev_mask] == [(2, 2, 64, 96)] * 2 and opt.flow_mix == (fallback == "mix")
        held.append(sorted(vars(opt)))
    assert held[0] == held[1], "mix holds what nearer holds"
