"""The clip of the scene-cut tests (tests/test_video_cuts_cpu.py, tests/test_hip_video_cuts.py) and what both read from it: two synthetic
scenes of tests/video_clips.py joined, 10 frames with the cut between frames 4 and 5, and the scores ssm_amd.video.SceneCuts gives its
pairs through the host yardstick.

The scenes of clip_payloads move by (3, 2) pixels a frame under fine grain: a mean absolute luma difference of about 14 codes between
neighbours, half of what two unrelated scenes of that family differ by - too close for a score that is damped by its own change, and
nothing like footage.  So both scenes keep their motion and lose contrast, a dim one (Y = 16 + (Y - 16) // 4, codes 16 .. 70) before a
bright one (Y = 235 - (Y - 16) // 4, codes 181 .. 235), chroma as it is: neighbours differ by about 3.5 codes, the cut by about 160.

A plain helper module (no fixtures, no collection hooks), imported as tests/video_clips.py is.
"""
from fractions import Fraction

import numpy as np

from video_clips import V, clip_payloads

N_FRAMES, CUT = 10, 4                  # the cut pair is (CUT, CUT + 1)
SIZES = ((64, 96), (45, 71))           # the aligned size and the odd one of the GPU tests
THRESHOLD = Fraction(1, 10)            # between the largest score of a pair that is no cut and the cut's: see test_video_cuts_cpu.py


def cut_clip(h, w, siting=0):
    """[10, frame_bytes] uint8: frames 0 .. 4 the dim scene, 5 .. 9 the bright one."""
    a, b = clip_payloads(CUT + 1, h, w, siting, seed=5).copy(), clip_payloads(N_FRAMES - CUT - 1, h, w, siting, seed=6).copy()
    a[:, :h * w] = 16 + (a[:, :h * w] - 16) // 4
    b[:, :h * w] = 235 - (b[:, :h * w] - 16) // 4
    return np.concatenate([a, b])


def luma(payloads, h, w):
    return payloads[:, :h * w].reshape(-1, h, w)


def pair_scores(payloads, h, w, pairs=None, threshold=THRESHOLD):
    """[(i, is a cut, score)] of the pairs (i, i + 1) fed in order (all of them, or `pairs`: those a timeline runs), by the yardstick."""
    v = V()
    y = luma(payloads, h, w)
    pairs = list(range(len(payloads) - 1)) if pairs is None else list(pairs)
    sums = v.luma_sad_host(y[pairs], y[[i + 1 for i in pairs]])
    sc = v.SceneCuts(threshold)
    return [(i,) + sc.feed(int(s), h * w) for i, s in zip(pairs, sums)]
