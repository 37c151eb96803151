#!/usr/bin/env python3
"""Pre-decode a clip list: every clip of an ADOBE / NFS-format list of image files becomes one `.npy` of [T, H, W, 3] uint8 RGB, and a
matching list addresses its frames as `clip_00000.npy#k` (ssm_amd.data reads those through a memory map: no decoding while training).
This project's counterpart of the reference's scripts/utils/make_clips.py, which writes the lists of image files.

    python scripts/utils/pack_clips.py train_clips.txt packed/ packed/train_clips.txt

Point <DATASET>_DATA.TRAINPATHS of the ini at the new list.  A 57-frame 720p clip takes 158 MB.
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(os.path.dirname(HERE)),):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from ssm_amd.data import ClipReadError, frame_source, parse_counted_list  # noqa: E402


def pack_clips(list_path, out_dir, out_list):
    """Returns the number of clips written."""
    with open(list_path) as f:
        clips = parse_counted_list(f.readlines())
    os.makedirs(out_dir, exist_ok=True)
    lines = ["%d" % len(clips)]
    for i, paths in enumerate(clips):
        first = frame_source(paths[0])
        dst = os.path.abspath(os.path.join(out_dir, "clip_%05d.npy" % i))
        arr = np.lib.format.open_memmap(dst, mode="w+", dtype=np.uint8, shape=(len(paths),) + first.shape)
        for k, p in enumerate(paths):
            fr = first if k == 0 else frame_source(p)
            if fr.shape != first.shape:
                raise ClipReadError("%s: a %dx%d frame in a clip of %dx%d frames" % (p, fr.shape[0], fr.shape[1], first.shape[0], first.shape[1]))
            arr[k] = fr
        arr.flush()
        del arr
        lines.append("%d" % len(paths))
        lines.extend("%s#%d" % (dst, k) for k in range(len(paths)))
    with open(out_list, "w") as f:
        f.write("\n".join(lines) + "\n")
    return len(clips)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("clip_list", help="ADOBE / NFS-format list of image files")
    ap.add_argument("out_dir", help="directory for the .npy clips")
    ap.add_argument("out_list", help="the list to write")
    a = ap.parse_args()
    print("%d clips packed" % pack_clips(a.clip_list, a.out_dir, a.out_list))
