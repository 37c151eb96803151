"""No-GPU checks of the one block-pass loop under the fixed grid, the fields and the hold-out scorer (ssm_amd.video.read_blocks, DESIGN
3.12) - a fake reader, a real PassRing, writers that keep lists - and of the clips of the stream digests (tests/video_stream_clips.py,
tests/test_hip_video_stream_digest.py): on the host, the option clips hold exactly one scene cut and, in every pair, static blocks but
never static blocks only, so a digest cannot agree with the recorded one by an option doing nothing."""
import json
import os
import sys
from fractions import Fraction as Fr

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import video_cut_clips as C  # noqa: E402
import video_stream_clips as K  # noqa: E402

DEPTH = 3


class Frames:
    """A reader of n one-byte frames: frame i holds i."""

    def __init__(self, n):
        self.n, self.read = n, 0

    def read_frame_into(self, buf):
        if self.read == self.n:
            return False
        buf[...] = self.read
        self.read += 1
        return True


class Keep:
    def __init__(self, fail_at=None):
        self.frames, self.fail_at = [], fail_at

    def write_frame(self, buf):
        if len(self.frames) == self.fail_at:
            raise RuntimeError("the disk is full")
        self.frames.append(int(buf[0]))


def lengths(pb):
    return (0, 1, pb, pb + 1, 2 * pb + 1, 2 * pb + 2)


def run_blocks(reader, pb, writer, read_unit=None, np_in=None):
    """A block mode without its GPU work: frame 0 ahead of pass 0, then read_blocks; -> [(valid, the pass's input rows)] as issued."""
    from ssm_amd.video import PassRing, first_frame, read_blocks
    np_in = [np.full((pb, 1), 255, np.uint8) for _ in range(DEPTH)] if np_in is None else np_in
    first, issued = np.zeros(1, np.uint8), []
    first_frame(reader, first)
    with PassRing(DEPTH, writer) as ring:
        ring.hand(None, None, [first])

        def issue(r, valid):
            issued.append((valid, np_in[r][:, 0].tolist()))
            ring.hand(r, None, [np_in[r][i] for i in range(valid)])

        read_blocks(ring, pb, np_in, read_unit or (lambda r, i: reader.read_frame_into(np_in[r][i])), issue)
        run_blocks.ring = ring
    return issued


@pytest.mark.parametrize("pb", (1, 2, 3))
def test_passes_of_the_block_loop(pb):
    from ssm_amd.video import Y4MError
    for n in lengths(pb):
        writer = Keep()
        if n == 0:
            with pytest.raises(Y4MError, match="the Y4M stream holds no frame"):
                run_blocks(Frames(0), pb, writer)
            assert writer.frames == []
            continue
        issued = run_blocks(Frames(n), pb, writer)
        full, rest = divmod(n - 1, pb)
        assert [valid for valid, _ in issued] == [pb] * full + [rest], "every pass but the last is full; the last may be short or empty"
        assert writer.frames == list(range(n)), "the frames come out in order, each once"
        for p, (valid, rows) in enumerate(issued[:full]):
            assert rows == list(range(1 + p * pb, 1 + (p + 1) * pb))
        if rest:
            rows = issued[-1][1]
            assert rows[:rest] == list(range(n - rest, n)) and rows[rest:] == [n - 1] * (pb - rest), "a short pass is filled with its last frame"
        assert run_blocks.ring.free.qsize() == DEPTH


@pytest.mark.parametrize("pb", (1, 2, 3))
def test_a_failing_writer_stops_the_block_loop(pb):
    n, k = 400, 5
    reader, writer = Frames(n), Keep(fail_at=k)
    with pytest.raises(RuntimeError, match="the disk is full"):
        run_blocks(reader, pb, writer)
    ring = run_blocks.ring
    assert writer.frames == list(range(k)), "nothing is written after the failure"
    # the producer looks at `failure` once a pass; the thread frees no slot between the failure and its note, so at most the passes in
    # the ring and the one being read lie between the failing frame and the stop
    assert reader.read <= k + 1 + (DEPTH + 1) * pb < n, "reading stops"
    assert ring.free.qsize() == DEPTH and len(ring.failure) == 1, "every slot comes back"


@pytest.mark.parametrize("hold", (2, 3))
@pytest.mark.parametrize("pb", (1, 2, 3))
def test_the_scorers_group_reader(pb, hold):
    """The hold-out scorer's unit is a group of `hold` frames: kept, frames_read and trailing are hold_out_plan's at every length."""
    from types import SimpleNamespace
    from ssm_amd.video_score import group_reader, hold_out_plan
    nt = hold - 1
    for n in sorted(set(lengths(pb)) | {1 + hold * groups + t for groups in (pb - 1, pb, 2 * pb, 2 * pb + 1) for t in range(hold)}):
        if n == 0:
            continue
        res = SimpleNamespace(frames_read=1, kept=1, trailing=0)
        reader, writer = Frames(n), Keep()
        np_in = [np.full((pb, 1), 255, np.uint8) for _ in range(DEPTH)]
        np_held = [np.full((pb * nt, 1), 255, np.uint8) for _ in range(DEPTH)]
        held = []

        def read_unit(r, i, read=group_reader(reader, res, hold, np_held, np_in)):
            whole = read(r, i)
            if whole:
                held.extend(np_held[r][i * nt:(i + 1) * nt, 0].tolist())
            return whole

        issued = run_blocks(reader, pb, writer, read_unit, np_in)
        kept, scored, trailing = hold_out_plan(n, hold)
        res.kept += sum(valid for valid, _ in issued)
        assert (res.kept, res.frames_read, res.trailing) == (len(kept), n, len(trailing)), n
        assert writer.frames == kept and held == [i for i, _ in scored]
        full, rest = divmod(len(kept) - 1, pb)
        assert [valid for valid, _ in issued] == [pb] * full + [rest]


def test_the_fixture_holds_the_cases():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "video_stream_digest.json")) as f:
        recorded = json.load(f)
    assert sorted(recorded["cases"]) == K.case_keys() and len(recorded["cases"]) == 296
    assert all(len(d) == 64 for d in recorded["cases"].values())


def option_clips():
    for h, w in C.SIZES:
        for n in sorted({n for pb in K.BATCHES for n in K.fixed_lengths(pb)}):
            yield h, w, K.option_clip(h, w, n), None
        for name, step in (("75", Fr(2, 5)), ("5/2", Fr(5, 2)), ("4/3", Fr(4, 3))):
            yield h, w, K.option_clip(h, w, K.TIMELINE_FRAMES, K.TIMELINE_CUT), step


def test_the_option_clips_have_one_cut_and_some_static_blocks():
    from ssm_amd.video import Timeline, block_sad_host, static_blocks, static_paste_host
    for h, w, clip, step in option_clips():
        pairs = list(range(len(clip) - 1))
        assert [i for i, cut, _ in C.pair_scores(clip, h, w) if cut] == [(len(clip) - 1) // 2 if step is None else K.TIMELINE_CUT]
        if step is not None:          # the pairs a timeline runs, fed in their order: the same single cut
            tl = Timeline(step)
            pairs = [i for i in pairs if tl.count(i) > 0]
            assert K.TIMELINE_CUT in pairs and [i for i, cut, _ in C.pair_scores(clip, h, w, pairs) if cut] == [K.TIMELINE_CUT]
        blocks = static_blocks(h, w)
        moving = block_sad_host(clip[:-1], clip[1:], h, w, 0, 8, lo=0)[:, 0, 1]          # luma blocks that differ at all
        _, static = static_paste_host(np.zeros((len(clip) - 1, 1, clip.shape[1]), np.uint8), clip[:-1], clip[1:], h, w, 0, 8, 0)
        assert all(0 < int(s) <= blocks - int(m) < blocks for s, m in zip(static, moving)), (h, w, static.tolist(), moving.tolist())


def test_the_uneven_timeline_takes_two_luma_calls_in_a_pass():
    """speed = 4/3 at pairs_per_batch 3: a pass's pairs do not step evenly, which 5/2 never gives (a ring slot's rows run out first)."""
    from ssm_amd.video import PassPlanner, Timeline, sad_runs

    def runs_of(step, pb):
        plan, out = PassPlanner(Timeline(step), pb, 2 * pb + 2), []
        for closed in [plan.frame() for _ in range(K.TIMELINE_FRAMES)] + [plan.end()]:
            if closed is not None and closed[1]:
                rights = [1 + row + (1 if own else 0) for row, own, _ in closed[1]]
                lefts = [1 + row if own else (rights[p - 1] if p else 0) for p, (row, own, _) in enumerate(closed[1])]
                out.append(len(sad_runs(lefts, rights)))
        return out

    assert max(runs_of(Fr(4, 3), 3)) == 2 and K.TIMELINES[K.UNEVEN] == {"speed": "4/3"}
    assert all(max(runs_of(step, pb)) == 1 for step in (Fr(2, 5), Fr(5, 2)) for pb in K.BATCHES)
