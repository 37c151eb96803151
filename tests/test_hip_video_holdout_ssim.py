"""HoldOutScorer(ssim=True, mix=True) end to end on the GPU (ssm_amd/video_score.py).  The options add columns and change
nothing else: `frames` and the written bytes are those of a run with both off; the `mix` sums are the yardsticks (payload_mix_host, then
plane_sse_host and plane_ssim_host) applied on the host to the INPUT payloads; the SSIM sums of `model` are plane_ssim_host on the output of
the existing VideoInterpolator(upsample_rate=hold) run on the decimated clip, those of `nearest` the yardstick on the input bytes.  Every
sum is an integer and must be EQUAL.  Synthetic weights: the numbers say nothing about quality."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from video_clips import S, V, clip_payloads, deep_payloads, reference, score, synthetic_model, y4m  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def model():
    return synthetic_model(DEV)


def three(x):
    return tuple(int(t) for t in x[0])


CASES = [("420jpeg", 9, 2, 1), ("420jpeg", 9, 2, 2), ("420jpeg", 13, 4, 1), ("420jpeg", 13, 4, 2), ("422p10", 7, 2, 1), ("422p10", 7, 2, 2)]


@pytest.mark.parametrize("tag,n,hold,pb", CASES)
def test_the_new_columns_equal_their_yardsticks_and_nothing_else_moves(model, tag, n, hold, pb):
    cfg, m = model
    v, s = V(), S()
    h, w = 64, 96
    layout, bits = v.EXTENDED_TAGS[tag]
    payloads = deep_payloads(n, h, w, tag) if bits > 8 else clip_payloads(n, h, w, layout)
    kw = dict(n_streams=2, pairs_per_batch=pb)
    off, off_bytes = score(m, cfg, payloads, h, w, tag, hold, **kw)
    seen, seen_more = [], []
    on, on_bytes = score(m, cfg, payloads, h, w, tag, hold, ssim=True, mix=True,
                         callbacks=dict(on_frame=lambda *row: seen.append(row), on_scores=lambda i, k, more: seen_more.append((i, k, more))), **kw)
    assert on.frames == off.frames and seen == on.frames and all(len(f) == 4 for f in on.frames)
    assert np.array_equal(on_bytes, off_bytes), "the written bytes are those of the run without the options"
    assert (on.frames_read, on.kept, on.trailing, on.written) == (off.frames_read, off.kept, off.trailing, off.written)
    assert off.more == [] and len(on.more) == len(on.frames) and [(i, k) for i, k, _ in seen_more] == [(f[0], f[1]) for f in on.frames]
    assert [x[2] for x in seen_more] == on.more
    assert on.windows == s.plane_windows(h, w, layout) and all(c > 0 for c in on.windows)
    ref = reference(m, cfg, payloads, h, w, tag, hold, **kw)
    assert np.array_equal(ref, off_bytes)
    for (i, k, _, _), more in zip(on.frames, on.more):
        left, right = i - k, i - k + hold
        near = left if 2 * k < hold else right
        held = payloads[i:i + 1]
        mixed = s.payload_mix_host(payloads[left:left + 1], payloads[right:right + 1], 1, k, 0, hold, bits)
        assert sorted(more) == ["sse", "ssim"] and sorted(more["sse"]) == ["mix"] and sorted(more["ssim"]) == ["mix", "model", "nearest"]
        assert more["sse"]["mix"] == three(s.plane_sse_host(mixed, held, h, w, layout, bits)), (i, k)
        assert more["ssim"]["mix"] == three(s.plane_ssim_host(mixed, held, h, w, layout, bits)), (i, k)
        assert more["ssim"]["nearest"] == three(s.plane_ssim_host(held, payloads[near:near + 1], h, w, layout, bits)), (i, k)
        assert more["ssim"]["model"] == three(s.plane_ssim_host(ref[i:i + 1], held, h, w, layout, bits)), (i, k)
        assert all(type(x) is int for col in more["ssim"].values() for x in col)
    # the report: pooled by sums and window counts
    p = on.pooled()
    cnt = [c * len(on.frames) for c in on.windows]
    assert p["model"] == off.pooled()["model"] and p["nearest"] == off.pooled()["nearest"]
    assert p["ssim"]["model"]["y"] == s.ssim_value(sum(x["ssim"]["model"][0] for x in on.more), cnt[0])
    assert p["ssim"]["mix"]["avg"] == s.ssim_value(sum(sum(x["ssim"]["mix"]) for x in on.more), sum(cnt))
    assert p["mix"]["y"] == s.psnr(sum(x["sse"]["mix"][0] for x in on.more), on.samples[0] * len(on.frames), bits)
    assert all(-1.0 <= val <= 1.0 for col in p["ssim"].values() for val in col.values())
    assert on.table().split("\n")[:len(off.table().split("\n"))] == off.table().split("\n")
    assert [ln[:len(o)] for ln, o in zip(on.stats_lines(), off.stats_lines())] == off.stats_lines()


def test_one_option_at_a_time(model):
    cfg, m = model
    s = S()
    h, w, hold = 64, 96, 4
    payloads = clip_payloads(9, h, w, 0)
    both, _ = score(m, cfg, payloads, h, w, "420jpeg", hold, ssim=True, mix=True)
    only_ssim, _ = score(m, cfg, payloads, h, w, "420jpeg", hold, ssim=True)
    only_mix, _ = score(m, cfg, payloads, h, w, "420jpeg", hold, mix=True)
    assert only_ssim.frames == only_mix.frames == both.frames
    assert [x["ssim"] for x in only_ssim.more] == [{c: x["ssim"][c] for c in ("model", "nearest")} for x in both.more]
    assert [x for x in only_mix.more] == [{"sse": x["sse"]} for x in both.more]
    assert sorted(only_ssim.pooled()) == ["frames", "model", "nearest", "ssim"] and sorted(only_mix.pooled()) == ["frames", "mix", "model", "nearest"]
    assert "mix_y" not in only_ssim.table() and "SSIM" not in only_mix.table() and "mix_y" in only_mix.table()
    assert s.HoldOutScorer(m, cfg, 2).ssim is False and s.HoldOutScorer(m, cfg, 2).mix is False


@pytest.mark.parametrize("pb", [1, 2])
def test_trailing_frames_and_short_clips_are_reported_as_before(model, pb):
    cfg, m = model
    payloads = clip_payloads(11, 64, 96, 0)
    res, got = score(m, cfg, payloads, 64, 96, "420jpeg", 4, ssim=True, mix=True, n_streams=2, pairs_per_batch=pb)
    assert (res.frames_read, res.kept, res.trailing, res.scored) == (11, 3, 2, 6) and got.shape[0] == 9 and len(res.more) == 6
    assert "2 trailing and not scored" in res.table()
    for n in (1, 3):
        res, got = score(m, cfg, payloads[:n], 64, 96, "420jpeg", 4, ssim=True, mix=True, pairs_per_batch=pb)
        assert (res.frames_read, res.kept, res.trailing, res.scored, res.written) == (n, 1, n - 1, 0, 1) and res.more == []
        assert np.array_equal(got, payloads[:1])
        assert res.pooled() is None and res.stats_lines() == [] and "nothing scored" in res.table()
        off, _ = score(m, cfg, payloads[:n], 64, 96, "420jpeg", 4, pairs_per_batch=pb)
        assert res.table() == off.table()


def test_an_empty_stream_is_refused(model):
    cfg, m = model
    v = V()
    with pytest.raises(v.Y4MError, match="holds no frame"):
        score(m, cfg, clip_payloads(1, 64, 96, 0)[:0], 64, 96, "420jpeg", 2, ssim=True, mix=True)


def test_device_memory_is_flat_in_clip_length(model):
    cfg, m = model
    v, s = V(), S()
    h, w, hold = 64, 96, 4
    scorer = s.HoldOutScorer(m, cfg, hold, n_streams=2, pairs_per_batch=1, ssim=True, mix=True)
    peaks = []
    for n in (9, 9, 41):          # the first run also builds the plans
        data = y4m(clip_payloads(n, h, w, 0), h, w, "420jpeg")
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(DEV)
        r = v.Y4MReader(data, extended=True)
        with open(os.devnull, "wb") as sink:
            res = scorer.run(r, v.Y4MWriter.like(sink, r))
        assert res.scored == (n - 1) // hold * (hold - 1) == len(res.more)
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated(DEV))
    print("peak device memory: 9 frames %d B, 41 frames %d B" % (peaks[1], peaks[2]))
    assert peaks[2] <= peaks[1], peaks


def test_cli_ssim_and_mix(model, tmp_path, capsys):
    import evaluate_video
    cfg, m = model
    h, w, n, hold, tag = 40, 56, 6, 2, "422p10"
    payloads = deep_payloads(n, h, w, tag)
    src, ini, logf, stats = (str(tmp_path / x) for x in ("in.y4m", "cfg.ini", "log.txt", "frames.log"))
    with open(src, "wb") as f:
        f.write(y4m(payloads, h, w, tag).getvalue())
    with open(ini, "w") as f:
        cfg.write(f)
    base = ["-c", ini, "--expt", "t", "--log", logf, "--input", src, "--hold", str(hold)]
    plain = evaluate_video.main(base, model=m)
    default_out = capsys.readouterr().out
    res = evaluate_video.main(base + ["--ssim", "--mix", "--stats", stats], model=m)
    out = capsys.readouterr().out
    assert default_out == plain.table() + "\n" and out == res.table() + "\n" and res.frames == plain.frames
    first = default_out.split("\n")[:-1]
    assert out.split("\n")[:len(first)] == first, "the first lines are the default table's"
    rest = out.split("\n")[len(first):]
    assert any("mix_y" in ln and "mix_avg" in ln for ln in rest) and any("model_y" in ln and "near_y" in ln and "mix_y" in ln for ln in rest)
    assert any(ln.startswith("SSIM") and "pooled by windows" in ln for ln in rest)
    with open(stats) as f:
        lines = f.read().splitlines()
    assert lines == res.stats_lines() and len(lines) == 2 and " mix_psnr_y " in lines[0] and " ssim_y " in lines[0] and " mix_ssim_y " in lines[1]
