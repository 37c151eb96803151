#!/usr/bin/env python3
"""Record which option combinations of the streamed-video path a commit takes and which it refuses, with every refusal's full text.

    git worktree add /tmp/parent <commit>
    python tests/golden/make_video_refusals.py --tree /tmp/parent

The cases are those of tests/video_option_cases.py in THIS checkout; VideoInterpolator and scripts/interpolate_video.py are imported from
--tree, a clean checkout of the commit to record (its hash goes into the file).  Writes tests/golden/video_refusals.json: the distinct
outcomes once ("messages"; an entry is [exception type, message] for the constructor, the text handed to parser.error for the tool),
and per front end {case: index into them, or null where the combination is accepted}.  Needs no GPU."""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--tree", required=True, help="A clean checkout of the commit whose outcomes are recorded.")
    args = parser.parse_args()
    tree = os.path.abspath(args.tree)
    commit = subprocess.check_output(["git", "-C", tree, "rev-parse", "HEAD"], text=True).strip()
    if subprocess.check_output(["git", "-C", tree, "status", "--porcelain", "--untracked-files=no"], text=True).strip():
        sys.exit("%s has uncommitted changes: it is not the commit %s" % (tree, commit))
    pkg = os.path.join(tree, "superslomo-videointerpolation-pytorch_amd")
    sys.path[:0] = [os.path.join(ROOT, "tests"), pkg, os.path.join(pkg, "scripts")]
    import interpolate_video
    import video_option_cases as C
    from ssm_amd import video as V
    assert V.__file__.startswith(tree + os.sep) and interpolate_video.__file__.startswith(tree + os.sep), "the code under record is --tree's"
    messages, fronts = [], []
    for outcomes in C.outcomes(V, interpolate_video):
        front = {}
        for case, outcome in outcomes.items():
            if outcome is not None and outcome not in messages:
                messages.append(outcome)
            front[case] = None if outcome is None else messages.index(outcome)
        fronts.append(front)
    with open(os.path.join(HERE, "video_refusals.json"), "w") as f:
        json.dump({"commit": commit, "messages": messages, "api": fronts[0], "flags": fronts[1]}, f, indent=0, sort_keys=False)
        f.write("\n")
    print("%s: %d + %d cases, %d refused, %d distinct messages" % (commit, len(fronts[0]), len(fronts[1]),
                                                                     sum(v is not None for fr in fronts for v in fr.values()), len(messages)))


if __name__ == "__main__":
    main()
