"""ssm_frames_accumulate_light_fwd computes, bit for bit, what the commit noted in tests/golden/video_light_digest.json computed: SHA-256
digests of the whole accumulator buffer - the view's region and its poisoned surround - after one call, at the shapes of
tests/test_hip_shutter_light.py (the smallest at which the kernel's branches differ: one pixel per lane with partial blocks, four pixels
per lane, one pixel per lane by alignment alone), for the three curves, N in 1, 2, 5 (5: the remainder of the loop's unroll by 4), init
and encode 0 and 1, under the config's mean and std.  tests/test_hip_shutter_light.py holds the kernel to a bound against a float64
yardstick, which a reordered operation would pass; this pins the order.

    python tests/test_hip_shutter_light_digest.py --record [--commit ID]

writes the fixture (every case runs twice; two different digests and nothing is written; $SSM_VIDEO_LIGHT_DIGEST_OUT: another path to
write to).  The module uses only names the recorded commit has as well, so the same file records there and compares here."""
import hashlib
import json
import os
import sys
import zlib

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "video_light_digest.json")
NAMES = ["5x7", "6x12", "6x12 strided"]
CURVES = ["bt709", "srgb", "bt1886"]          # every curve ssm_amd.video has: test_fixture_covers_the_cases


def cases(name, curve):
    return [(name, curve, n, init, encode) for n in (1, 2, 5) for init in (0, 1) for encode in (0, 1)]


def key(case):
    return "%s|%s|N=%d|init=%d|encode=%d" % case


def run_case(case):
    """The digest of the accumulator's whole buffer after one call; the inputs come from a generator seeded by the case's key."""
    from ssm_amd import hipbind as hb
    from test_hip_shutter_light import values, views
    from test_video_light_cpu import MEAN, STD
    from video_clips import V
    name, curve, n, init, encode = case
    row = V().light_curve(curve)
    rng = np.random.default_rng(zlib.crc32(key(case).encode()))
    src, abuf, acc, _ = views(name, n)
    src.copy_(torch.from_numpy(values(rng, tuple(src.shape), MEAN, STD, row)))
    held = 0 if init else 3          # as tests/test_hip_shutter_light.py: an accumulator that continues holds sums of light in [0, 3]
    acc.copy_(torch.from_numpy((rng.uniform(0.0, 1.0, tuple(acc.shape)) * held).astype(np.float32)))
    scale = np.float32(1.0 / (held + n)) if encode else np.float32(1.0)
    assert hb.frames_accumulate_light(src, acc, init, scale, MEAN, STD, row, encode) is acc
    torch.cuda.synchronize()
    return hashlib.sha256(abuf.cpu().numpy().tobytes()).hexdigest()


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_covers_the_cases(recorded):
    from video_clips import V
    assert sorted(CURVES) == sorted(V().LIGHT_CURVES)
    want = sorted(key(c) for name in NAMES for curve in CURVES for c in cases(name, curve))
    assert len(recorded["commit"]) >= 7 and len(want) == 108 and sorted(recorded["cases"]) == want


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("name", NAMES)
def test_light_kernel_is_bitwise_what_was_recorded(recorded, name, curve):
    got = {key(c): run_case(c) for c in cases(name, curve)}
    differ = sorted(k for k in got if got[k] != recorded["cases"][k])
    assert not differ, "%d of %d digests differ from commit %s: %s" % (len(differ), len(got), recorded["commit"], differ)


def record(commit):
    out = {"commit": commit, "cases": {}}
    for name in NAMES:
        for curve in CURVES:
            for c in cases(name, curve):
                a, b = run_case(c), run_case(c)
                if a != b:
                    raise SystemExit("case %s is not repeatable: %s / %s - nothing written" % (key(c), a, b))
                out["cases"][key(c)] = a
    path = os.environ.get("SSM_VIDEO_LIGHT_DIGEST_OUT", FIXTURE)
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %d digests to %s" % (len(out["cases"]), path))


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "superslomo-videointerpolation-pytorch_amd")
    for p in (root, pkg, os.path.join(pkg, "scripts")):
        if p not in sys.path:
            sys.path.insert(0, p)
    if "--record" not in sys.argv:
        raise SystemExit("usage: python tests/test_hip_shutter_light_digest.py --record [--commit ID]")
    record(sys.argv[sys.argv.index("--commit") + 1] if "--commit" in sys.argv else "unknown")
