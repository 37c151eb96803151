"""The clips and the case list of the stream digests (tests/test_hip_video_stream_digest.py, tests/test_video_block_loop_cpu.py): every
run loop of the streamed video path on clips small enough to run in a blink, at every n_streams and pairs_per_batch at which a loop takes
another turn.

One clip family serves the options: option_clip(h, w, n, cut) is the recipe of tests/video_cut_clips.py - a dim scene up to frame `cut`, a
bright one behind it - with the top left quarter of its 8 x 8 blocks, luma and the chroma under them, made frame 0's in every frame (what
tools/bench_static.py's keep_quarter does at 720p).  So one pair is a scene cut, every pair has static blocks, and no pair has only
static blocks: neither option can agree with a recorded digest by doing nothing.  tests/test_video_block_loop_cpu.py asserts that.

A plain helper module (no fixtures, no collection hooks), imported as tests/video_clips.py is; it uses only names of the public surface."""
import numpy as np

from video_clips import V, clip_payloads
from video_cut_clips import SIZES, THRESHOLD

STREAMS, BATCHES = (1, 2), (1, 2, 3)
OPTIONS = {"none": {}, "cut": {"scene_cut": THRESHOLD}, "static": {"static": 0}, "both": {"scene_cut": THRESHOLD, "static": 0}}
TIMELINES = {"75": {"target_rate": (75, 1)}, "5/2": {"speed": "5/2"}, "4/3": {"speed": "4/3"}}          # from 30 frames a second
# 75: every pair runs.  5/2 runs pairs 2, 7 and 12 of 15 and skips frames; its passes never hold more than two pairs (a ring slot's rows
# run out first), so ssm_luma_sad_fwd gets one call a pass.  4/3 runs pairs 1, 2, 5, 6, 9, 10, 13, 14: at pairs_per_batch 3 a pass holds
# pairs (1, 2, 5) or (6, 9, 10), whose rows do not step evenly - sad_runs then makes two calls.  It runs with both options only.
# Pair (2, 3) runs under all three.
TIMELINE_FRAMES, TIMELINE_CUT, UNEVEN = 16, 2, "4/3"
BOXED = {"420jpeg": (None, THRESHOLD), "422p10": (None,)}          # tag -> its scene_cut values: scene cuts are refused above 8 bits
HOLD, SCORER_FRAMES = 3, (6, 7, 8)             # trailing 0, 1, 2
FIELD_FRAMES, OTHER_FRAMES = 5, 6


def keep_quarter(frames, h, w, siting=0):
    """The top left quarter of the blocks of every frame becomes frame 0's, in place: (h >> 4) x (w >> 4) blocks of (h >> 3) x (w >> 3)."""
    v = V()
    cr, cc = (8, 8) if siting == 2 else (8, 4) if siting == 3 else (4, 4)
    by, bx = (h >> 3) // 2, (w >> 3) // 2
    for plane, (rr, rc) in zip(v.split_planes(frames, h, w, siting, 8), ((8, 8), (cr, cc), (cr, cc))):
        plane[1:, :by * rr, :bx * rc] = plane[:1, :by * rr, :bx * rc]
    return frames


def two_scenes(h, w, n, cut, siting=0):
    """[n, frame_bytes] uint8: frames 0 .. cut a dim scene, the rest a bright one (tests/video_cut_clips.py's contrast rule)."""
    a, b = clip_payloads(cut + 1, h, w, siting, seed=5).copy(), clip_payloads(n - cut - 1, h, w, siting, seed=6).copy()
    a[:, :h * w] = 16 + (a[:, :h * w] - 16) // 4
    b[:, :h * w] = 235 - (b[:, :h * w] - 16) // 4
    return np.concatenate([a, b])


def option_clip(h, w, n, cut=None):
    """The clip of the option cases: n frames, the cut pair (cut, cut + 1) - in the middle by default -, a quarter of the blocks static."""
    return keep_quarter(two_scenes(h, w, n, (n - 1) // 2 if cut is None else cut), h, w)


def fixed_lengths(pb):
    """The clip lengths of the fixed grid at pairs_per_batch pb: 7 (the last pass is short at 2 and 3) and 2 pb + 1 (an empty last pass)."""
    return sorted({7, 2 * pb + 1})


def boxed_clip(tag):
    """The letterboxed clip of tests/video_active_clips.py in the format of a tag; the 8-bit clip's picture is two scenes, cut pair (2, 3)."""
    import video_active_clips as A
    if V().EXTENDED_TAGS[tag][1] > 8:
        return A.letterboxed(tag)[0]
    return A.boxed(two_scenes(A.H, A.W, OTHER_FRAMES, 2), tag)


def repeated_clip(h, w):
    """OTHER_FRAMES moving frames with frame 2 twice: one repaired repeat."""
    base = clip_payloads(OTHER_FRAMES, h, w, 0)
    return np.concatenate([base[:3], base[2:]])


def groups():
    """[(group, [case detail, ...])]: the runs of one pytest case at one (n_streams, pairs_per_batch), by the pb they depend on."""
    out = []
    for h, w in SIZES:
        out.append(("fixed-%dx%d" % (h, w), lambda pb: ["n=%d|%s" % (n, o) for n in fixed_lengths(pb) for o in OPTIONS]))
        out.append(("timeline-%dx%d" % (h, w), lambda pb: ["%s|%s" % (t, o) for t in TIMELINES for o in OPTIONS if t != UNEVEN or o == "both"]))
        out.append(("other-%dx%d" % (h, w), lambda pb, h=h: (["tff", "bff"] if h % 4 == 0 else []) + ["dedup", "shutter"]
                    + ["score n=%d" % n for n in SCORER_FRAMES]))
    out.append(("boxed", lambda pb: ["%s|%s|%s" % (tag, mode, "cut" if sc is not None else "none") for tag in BOXED
                                     for mode in ("fixed", "75") for sc in BOXED[tag]]))
    return out


def case_keys():
    """Every case as "group|n_streams|pairs_per_batch|detail", sorted: what the fixture holds."""
    return sorted("%s|%d|%d|%s" % (g, ns, pb, d) for g, details in groups() for ns in STREAMS for pb in BATCHES for d in details(pb))
