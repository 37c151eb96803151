#!/usr/bin/env python3
"""Stage-1 optical flow against Sintel ground truth: CLI of the reference's scripts/evaluate_optical_flow_results.py (same flags,
same log lines), MI355X-native inside:

  PNG -> uint8 on the GPU -> ingest kernel (normalise, zero rows to 448)             [ssm_amd.frames]
      -> FullModel.estimate_flow (stage 1 only; the reference runs the full model and keeps intermediate_outputs[0])
      -> crop rows 6:442 -> EPE and the share of pixels more than 3 px off           [ssm_amd.flow_eval]

Reads [SINTEL_EPE_DATA] ROOTDIR / SETTING and lists <ROOTDIR>/<setting>/<clip>/*.png and <ROOTDIR>/flow/<clip>/*.flo like
`Reader.read_clip_list` (scripts/utils/dataloaders/sintel_opticalflow.py:45-73).  Differences from the reference, on purpose: PIL
replaces cv2 (not a dependency here), no DataLoader workers, N_FRAMES must be 2, and --metrics device scores on the GPU
(csrc/ssm_flow.hip) instead of on a host copy of the flow (the default, --metrics host, is the reference's path).
"""
import argparse
import configparser
import glob
import logging
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from models import superslomo_r as ssm  # noqa: E402
from ssm_amd import flow_eval as FE  # noqa: E402
from ssm_amd import frames as F  # noqa: E402
from utils.flo_utils import read_flow  # noqa: E402

log = logging.getLogger(__name__)


def getargs(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("--log")
    parser.add_argument("-c", "--config")
    parser.add_argument("--metrics", choices=("host", "device"), default="host",
                        help="Score on a host copy of the flow (the reference's path) or on the GPU.")
    return parser.parse_args(argv)


def read_clip_list(cfg, n_frames=2):
    """[(image paths of one window, flow path)] over every clip (sintel_opticalflow.py:45-73)."""
    root = cfg.get("SINTEL_EPE_DATA", "ROOTDIR")
    setting = cfg.get("SINTEL_EPE_DATA", "SETTING").lower()
    log.info("Using render setting: %s" % setting)
    clips = sorted(glob.glob(os.path.join(root, setting, "*")))
    log.info("Found %s clips." % len(clips))
    data = []
    for clip_dir in clips:
        clip_name = os.path.basename(os.path.normpath(clip_dir))
        img_paths = sorted(glob.glob(clip_dir + "/*.png"))
        flow_paths = sorted(glob.glob(os.path.join(root, "flow", clip_name) + "/*.flo"))
        if "training" in root:
            assert len(img_paths) == len(flow_paths) + 1, "%s: %d images, %d flows" % (clip_name, len(img_paths), len(flow_paths))
        for input_indexes, target_idx in FE.sintel_windows(len(img_paths), n_frames):
            data.append(([img_paths[i] for i in input_indexes], flow_paths[target_idx]))
    log.info("Found %s samples" % len(data))
    return data


def load_sample(img_paths, flow_path, cfg, device):
    """One loader item (sintel_opticalflow.py:98-131, batch 1): ([1,N,3,Hp,Wp] normalised input on the device, [1,H,W,2] ground truth)."""
    from PIL import Image
    frames = torch.from_numpy(np.stack([np.asarray(Image.open(p).convert("RGB")) for p in img_paths])).to(device)
    return F.frames_from_u8(frames, cfg, pad_before_norm=False)[None], torch.from_numpy(read_flow(flow_path))[None]


def main(argv=None, model=None):
    """Returns (mean EPE, mean share of pixels more than 3 px off) over all samples."""
    args = getargs(argv)
    logging.basicConfig(filename=args.log, level=logging.INFO)
    config = configparser.RawConfigParser()
    if not config.read(args.config):
        raise FileNotFoundError(args.config)
    logging.info("Read config")
    n_frames = config.getint("TRAIN", "N_FRAMES")
    if n_frames != 2:
        raise NotImplementedError("N_FRAMES=%d needs the recurrent bottleneck (unpinned upstream); use N_FRAMES=2" % n_frames)
    model = (model if model is not None else ssm.FullModel(config)).cuda().eval()
    device = next(model.parameters()).device
    data = read_clip_list(config, n_frames)
    if not data:
        raise FileNotFoundError("no samples under %s" % config.get("SINTEL_EPE_DATA", "ROOTDIR"))
    h, w = read_flow(data[0][1]).shape[:2]          # one frame size per data set (436 x 1024 for Sintel)
    ev = FE.FlowEvaluator(config, model, h, w, metrics=args.metrics)
    ev.run_evaluation((load_sample(imgs, flo, config, device) for imgs, flo in data), log=log, total=len(data))
    log.info("Final average: EPE: %.3f 3_pct_error: %.3f" % ev.means())
    return ev.means()


if __name__ == "__main__":
    main()
