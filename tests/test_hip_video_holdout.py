"""HoldOutScorer end to end on the GPU (ssm_amd/video_score.py): the clip scored against its own held-out frames.  The yardstick
is the EXISTING VideoInterpolator(upsample_rate=hold) run on the decimated clip with the same n_streams and pairs_per_batch: the scorer's
`model` sums equal plane_sse_host of that output's synthesised frames against the held-out frames, `nearest` equals the yardstick on the
input bytes, and with a writer the scorer's output is that run's output byte for byte.  Synthetic weights: the numbers say nothing about
quality."""
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from video_clips import S, V, clip_payloads, deep_payloads, frames_of, reference, score, synthetic_model, y4m  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def model():
    return synthetic_model(DEV)


def nearest_rows(payloads, h, w, layout, bits, hold):
    """(i, k, the yardstick's sums of frame i against the nearer kept frame) on the input bytes."""
    s = S()
    _, held, _ = s.hold_out_plan(len(payloads), hold)
    rows = []
    for i, k in held:
        near = i - k if 2 * k < hold else i - k + hold
        rows.append((i, k, tuple(int(x) for x in s.plane_sse_host(payloads[i:i + 1], payloads[near:near + 1], h, w, layout, bits)[0])))
    return rows


CASES = [("420jpeg", 9, 2, 1), ("420jpeg", 9, 2, 2), ("420jpeg", 13, 4, 1), ("420jpeg", 13, 4, 2),          # 13 at hold 4, two pairs a pass: the
         ("422p10", 7, 2, 1), ("422p10", 7, 2, 2)]                                                              # stream ends inside the second pass; so does 7 at hold 2


@pytest.mark.parametrize("tag,n,hold,pb", CASES)
def test_scores_are_those_of_the_existing_tool_on_the_decimated_clip(model, tag, n, hold, pb):
    cfg, m = model
    v, s = V(), S()
    h, w = 64, 96
    layout, bits = v.EXTENDED_TAGS[tag]
    payloads = deep_payloads(n, h, w, tag) if bits > 8 else clip_payloads(n, h, w, layout)
    ref = reference(m, cfg, payloads, h, w, tag, hold, n_streams=2, pairs_per_batch=pb)
    seen = []
    r = v.Y4MReader(y4m(payloads, h, w, tag), extended=True)
    sink = io.BytesIO()
    wr = v.Y4MWriter.like(sink, r)
    res = s.HoldOutScorer(m, cfg, hold, n_streams=2, pairs_per_batch=pb).run(r, wr, on_frame=lambda *row: seen.append(row))
    got = frames_of(sink.getvalue())
    kept, held, trailing = s.hold_out_plan(n, hold)
    assert (res.frames_read, res.kept, res.trailing, res.scored, res.written) == (n, len(kept), len(trailing), len(held), ref.shape[0])
    assert np.array_equal(got, ref), "with a writer: the existing run's output, byte for byte"
    assert np.array_equal(got[::hold], payloads[kept]), "kept frames as their own bytes"
    assert [(f[0], f[1]) for f in res.frames] == held and seen == res.frames
    near = nearest_rows(payloads, h, w, layout, bits, hold)
    for (i, k, model_sse, nearest_sse), (_, _, want_near) in zip(res.frames, near):
        want_model = tuple(int(x) for x in s.plane_sse_host(ref[i:i + 1], payloads[i:i + 1], h, w, layout, bits)[0])
        assert model_sse == want_model, (i, k)
        assert nearest_sse == want_near, (i, k)
        assert all(type(x) is int for x in model_sse + nearest_sse)
    assert sum(f[3][0] for f in res.frames) > 0, "the clip moves"
    # the report: pooled sums, not a mean of dB
    smp = s.plane_samples(h, w, layout)
    allk = res.pooled()
    assert allk["frames"] == len(held)
    assert allk["model"]["y"] == s.psnr(sum(f[2][0] for f in res.frames), smp[0] * len(held), bits)
    assert allk["nearest"]["avg"] == s.psnr(sum(sum(f[3]) for f in res.frames), sum(smp) * len(held), bits)
    assert res.worst() == min((s.psnr(f[2][0], smp[0], bits), f[0]) for f in res.frames)
    assert len(res.stats_lines()) == len(held) and ("%d/%d" % (hold - 1, hold)) in res.table()


def test_without_a_writer_the_scores_are_the_same(model):
    cfg, m = model
    payloads = clip_payloads(9, 64, 96, 0)
    with_w, _ = score(m, cfg, payloads, 64, 96, "420jpeg", 4, n_streams=2, pairs_per_batch=1)
    without, none = score(m, cfg, payloads, 64, 96, "420jpeg", 4, write=False, n_streams=2, pairs_per_batch=1)
    assert none is None and without.frames == with_w.frames and without.written == with_w.written == 9


@pytest.mark.parametrize("pb", [1, 2])
def test_trailing_frames_are_read_and_not_scored(model, pb):
    cfg, m = model
    payloads = clip_payloads(11, 64, 96, 0)
    res, got = score(m, cfg, payloads, 64, 96, "420jpeg", 4, n_streams=2, pairs_per_batch=pb)
    assert (res.frames_read, res.kept, res.trailing, res.scored) == (11, 3, 2, 6) and got.shape[0] == 9
    assert "2 trailing and not scored" in res.table()


@pytest.mark.parametrize("n", [1, 3, 4])
def test_a_clip_of_at_most_hold_frames_scores_nothing_and_says_so(model, n):
    cfg, m = model
    payloads = clip_payloads(n, 64, 96, 0)
    res, got = score(m, cfg, payloads, 64, 96, "420jpeg", 4)
    assert (res.frames_read, res.kept, res.trailing, res.scored, res.written) == (n, 1, n - 1, 0, 1)
    assert np.array_equal(got, payloads[:1]), "frame 0 goes out as _run_fixed writes it"
    assert res.pooled() is None and res.worst() is None and res.stats_lines() == [] and "nothing scored" in res.table()


def test_an_empty_stream_is_refused_as_run_fixed_refuses_it(model):
    cfg, m = model
    v = V()
    empty = clip_payloads(1, 64, 96, 0)[:0]
    with pytest.raises(v.Y4MError, match="holds no frame"):
        score(m, cfg, empty, 64, 96, "420jpeg", 2)
    r = v.Y4MReader(y4m(empty, 64, 96, "420jpeg"), extended=True)
    with pytest.raises(v.Y4MError, match="holds no frame"):
        v.VideoInterpolator(m, cfg, upsample_rate=2).run(r, v.Y4MWriter.like(io.BytesIO(), r))


def test_coarse_flow_and_tiles_run_to_the_end_with_the_same_nearest_sums(model):
    cfg, m = model
    h, w, hold = 120, 180, 2
    payloads = clip_payloads(5, h, w, 0)
    near = nearest_rows(payloads, h, w, 0, 8, hold)
    plain, _ = score(m, cfg, payloads, h, w, "420jpeg", hold, write=False)
    for kw in (dict(flow_scale=2), dict(tile=(64, 96), halo=32, blend=8)):
        res, _ = score(m, cfg, payloads, h, w, "420jpeg", hold, write=False, **kw)
        assert [(f[0], f[1], f[3]) for f in res.frames] == near == [(f[0], f[1], f[3]) for f in plain.frames], kw
        assert res.scored == 2 and all(sum(f[2]) > 0 for f in res.frames)


def test_options_without_a_held_out_counterpart_are_not_offered(model):
    cfg, m = model
    for kw in (dict(target_rate=(60, 1)), dict(speed=0.5), dict(shutter=0.5), dict(scene_cut=0.1)):
        with pytest.raises(TypeError):
            S().HoldOutScorer(m, cfg, 2, **kw)
    for hold in (1, 0, 2.5, True):
        with pytest.raises(ValueError, match="hold must be a whole number, at least 2"):
            S().HoldOutScorer(m, cfg, hold)


def test_cli_end_to_end_422p10(model, tmp_path, capsys):
    import evaluate_video
    cfg, m = model
    v, s = V(), S()
    h, w, n, hold, tag = 40, 56, 6, 2, "422p10"
    payloads = deep_payloads(n, h, w, tag)
    src, dst, ini, logf, stats = (str(tmp_path / x) for x in ("in.y4m", "out.y4m", "cfg.ini", "log.txt", "frames.log"))
    with open(src, "wb") as f:
        f.write(y4m(payloads, h, w, tag).getvalue())
    with open(ini, "w") as f:
        cfg.write(f)
    res = evaluate_video.main(["-c", ini, "--expt", "t", "--log", logf, "--input", src, "--hold", str(hold), "--stats", stats, "--output", dst],
                              model=m)
    assert (res.frames_read, res.kept, res.scored, res.trailing, res.written) == (6, 3, 2, 1, 5)
    with open(dst, "rb") as f:
        data = f.read()
    assert b" C422p10" in data.split(b"\n", 1)[0]
    got = frames_of(data)
    assert np.array_equal(got, reference(m, cfg, payloads, h, w, tag, hold)) and np.array_equal(got[::2], payloads[:5:2])
    with open(stats) as f:
        lines = f.read().splitlines()
    assert lines == res.stats_lines() and len(lines) == 2 and lines[0].startswith("n:1 k:1 mse_y ") and lines[1].startswith("n:3 k:1 mse_y ")
    out = capsys.readouterr().out
    assert out == res.table() + "\n" and "6 frames read, 3 kept, 2 scored, 1 trailing and not scored" in out and "peak 1023" in out
    assert [f[3] for f in res.frames] == [r[2] for r in nearest_rows(payloads, h, w, v.C422, 10, hold)]
