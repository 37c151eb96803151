#!/usr/bin/env python3
"""Interpolate a folder of frames; CLI of the reference's scripts/visualize_interpolation.py (same flags, same output
naming: <output_dir>/<expt>/images/img_00000.png, originals and intermediates interleaved), MI355X-native inside:

  PNG -> uint8 on the GPU -> ingest kernel (RGB, /255, normalise, pad to x32)        [ssm_amd.frames]
      -> FullModel.interpolate_many (stage 1 once per pair, all t batched, pairs on 2 HIP streams)
      -> egress kernel (crop, denormalise, uint8) -> PNG

Differences from the reference, on purpose: frames are cropped back to their original size before they are written
(the reference writes the zero-padded canvas), PIL replaces cv2 (not installed here), flow maps are saved as raw .npy
(with --flow_png also as the reference's colour-wheel PNGs, colour-coded on the GPU by ssm_amd.flow_eval.flow_to_rgb under the
reference's directory names; the files are true RGB, where the reference hands flow_to_image's RGB array to cv2.imwrite, which
takes it as BGR, so its colour maps have R and B swapped), and N_FRAMES must be 2 (CONV bottleneck).
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
from ssm_amd import evaluation as E  # noqa: E402
from ssm_amd import frames as F  # noqa: E402
from ssm_amd import tiles as T  # noqa: E402

log = logging.getLogger(__name__)


def getargs(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("-c", "--config", required=True, default="config.ini", help="Path to config.ini file.")
    parser.add_argument("--expt", required=True, help="Experiment Name.")
    parser.add_argument("--log", required=True, help="Path to logfile.")
    parser.add_argument("--input_dir", required=True, help="Directory with input images.")
    parser.add_argument("--img_type", required=True, help="Image type")
    parser.add_argument("--is_fps_240", action="store_true", help="Is input footage 240 fps?")
    parser.add_argument("--upsample_rate", type=int, default=8,
                        help="Integer upsampling rate. For 30FPS -> 240FP, use 8. For 1080FPS, use 36.")
    parser.add_argument("--show_intermediate_outputs", action="store_true",
                        help="Save occlusion maps, optical flow maps etc.?")
    parser.add_argument("--output_dir", required=True, help="Directory to output.")
    parser.add_argument("--flow_png", action="store_true",
                        help="With --show_intermediate_outputs: also save the flows as Middlebury colour-wheel PNGs.")
    parser.add_argument("--consistency_png", action="store_true",
                        help="With --show_intermediate_outputs: also save the forward-backward consistency masks of each pair's two "
                             "stage-1 flows as grey PNGs (0 consistent, 255 inconsistent, 128 leaves the picture), beside the flow maps.")
    parser.add_argument("--flow_scale", type=int, choices=(1, 2, 4), default=1,
                        help="Coarse-flow mode: run both U-Nets at 1/flow_scale of the frame size and synthesise at full size (an approximation "
                             "of the default output, not parity). Not with --show_intermediate_outputs. Default 1: off.")
    parser.add_argument("--tile", type=T.parse_tile, default=None, metavar="HxW",
                        help="Tiled mode: run the frame in overlapping windows with cores of H x W pixels (multiples of 32) and stitch them "
                             "(less memory; an approximation of the default output, not parity). Not with --show_intermediate_outputs. Default: off.")
    parser.add_argument("--halo", type=int, default=T.DEFAULT_HALO, help="With --tile: pixels of context around a tile's core (multiple of 32).")
    parser.add_argument("--blend", type=int, default=T.DEFAULT_BLEND,
                        help="With --tile: half width of the cross-fade over a seam (0 or a power of two >= 4, at most the halo).")
    return parser.parse_args(argv)


class Interpolator:
    def __init__(self, cfg, args, model=None):
        self.cfg, self.args = cfg, args
        self.n_frames = cfg.getint("TRAIN", "N_FRAMES")
        if self.n_frames != 2:
            raise NotImplementedError("N_FRAMES=%d needs the recurrent bottleneck (unpinned upstream); use N_FRAMES=2"
                                      % self.n_frames)
        self.model = (model if model is not None else ssm.FullModel(cfg)).cuda().eval()
        self.flow_scale = int(getattr(args, "flow_scale", 1))
        if self.flow_scale != 1 and args.show_intermediate_outputs:
            raise NotImplementedError("--flow_scale %d with --show_intermediate_outputs: the intermediates are those of the default mode "
                                      "(flow_scale 1)" % self.flow_scale)
        self.tile = getattr(args, "tile", None)
        self.halo, self.blend = getattr(args, "halo", T.DEFAULT_HALO), getattr(args, "blend", T.DEFAULT_BLEND)
        if self.tile is not None and args.show_intermediate_outputs:
            raise NotImplementedError("--tile %dx%d with --show_intermediate_outputs: the flows of different tiles are not one field"
                                      % tuple(self.tile))
        if self.tile is not None and self.flow_scale != 1:
            raise NotImplementedError("--tile %dx%d with --flow_scale %d: tiles are not available in the coarse-flow mode"
                                      % (tuple(self.tile) + (self.flow_scale,)))
        base = os.path.join(args.output_dir, args.expt)
        self.img_dir = os.path.join(base, "images")
        self.visibility_dir = os.path.join(base, "visibility_map")
        self.flow_dir = os.path.join(base, "refined_flow")
        os.makedirs(self.img_dir, exist_ok=True)
        if args.show_intermediate_outputs:
            os.makedirs(self.visibility_dir, exist_ok=True)
            os.makedirs(self.flow_dir, exist_ok=True)
        # the reference's colour-map directories (visualize_interpolation.py:90-103), opt-in
        self.flow_png = bool(getattr(args, "flow_png", False)) and args.show_intermediate_outputs
        self.flow_png_dirs = {name: os.path.join(base, name)
                              for name in ("estimated_flow_01", "estimated_flow_10", "refined_flow_t1", "refined_flow_t0")}
        if self.flow_png:
            for d in self.flow_png_dirs.values():
                os.makedirs(d, exist_ok=True)
        # the forward-backward consistency masks of a pair's two stage-1 flows (ssm_amd.flow_eval.flow_consistency), opt-in
        self.consistency_png = bool(getattr(args, "consistency_png", False)) and args.show_intermediate_outputs
        self.consistency_dirs = {d: os.path.join(base, name) for d, name in enumerate(("flow_consistency_01", "flow_consistency_10"))}
        if self.consistency_png:
            for d in self.consistency_dirs.values():
                os.makedirs(d, exist_ok=True)

    @staticmethod
    def load_frames(paths):
        from PIL import Image
        return torch.from_numpy(np.stack([np.asarray(Image.open(p).convert("RGB")) for p in paths]))   # [N,H,W,3] uint8

    def save(self, img_u8, count, out_dir, prefix="img"):
        from PIL import Image
        Image.fromarray(img_u8).save(os.path.join(out_dir, prefix + "_" + str(count).zfill(5) + ".png"))

    def save_flow_png(self, flow, h, w, top, left, count, name, prefix):
        """save_img_from_tensor(..., flo_img=True) (visualize_interpolation.py:223-232): the cropped [1,2,*,*] flow as a colour map."""
        from ssm_amd.flow_eval import flow_to_rgb
        self.save(flow_to_rgb(flow, h, w, top, left)[0].cpu().numpy(), count, self.flow_png_dirs[name], prefix)

    def save_consistency_png(self, flow01, flow10, h, w, top, left, count):
        """The two masks of a pair - 0 consistent, 1 inconsistent, 2 leaves - as grey 0 / 255 / 128, at the defaults FLOW_ALPHA, FLOW_BETA
        (a convention of the literature, not backed by a measurement here)."""
        from ssm_amd.flow_eval import flow_consistency
        _, mask = flow_consistency(torch.cat([flow01, flow10], 1).contiguous(), h, w, top, left, want_mask=True)
        grey = torch.tensor([0, 255, 128], dtype=torch.uint8, device=mask.device)[mask[0].long()].cpu().numpy()
        for d, prefix in enumerate(("Consistency_01", "Consistency_10")):
            self.save(grey[d], count, self.consistency_dirs[d], prefix)

    @torch.no_grad()
    def interpolate_frames(self):
        a = self.args
        paths = sorted(glob.glob(os.path.join(a.input_dir, "*." + a.img_type.lower())))
        log.info("Looking for %s images in %s. 240 FPS: %s. Found %d.", a.img_type, a.input_dir, a.is_fps_240, len(paths))
        if len(paths) < 2:
            raise FileNotFoundError("need at least two *.%s frames in %s" % (a.img_type.lower(), a.input_dir))
        windows = list(E.sliding_window(len(paths), self.n_frames, a.is_fps_240))
        used = sorted({i for w in windows for i in w})
        frames = self.load_frames([paths[i] for i in used]).cuda()
        pos = {i: k for k, i in enumerate(used)}
        h, w = frames.shape[1:3]
        x = F.frames_from_u8(frames, self.cfg, pad_before_norm=True, multiple=32 * self.flow_scale)       # visualiser convention (:76-87,:137)
        ts = E.t_values(a.upsample_rate)
        count = 0
        pairs = [torch.stack([x[pos[w0]], x[pos[w1]]])[None] for w0, w1 in windows]
        if a.show_intermediate_outputs:          # per-t forward keeps the reference's tuple of intermediates
            outs = []
            for pr in pairs:
                per_t = []
                for t in ts:
                    img, inter = self.model(pr, torch.full((1, 1, 1, 1, 1), t, device=pr.device), inference_mode=True)
                    per_t.append((img, inter))
                outs.append(per_t)
        else:
            outs = self.model.interpolate_many(pairs, ts, flow_scale=self.flow_scale, tile=self.tile, halo=self.halo, blend=self.blend)
        frames_cpu = frames.cpu().numpy()
        for k, (w0, w1) in enumerate(windows):
            self.save(frames_cpu[pos[w0]], count, self.img_dir)
            count += 1
            if a.show_intermediate_outputs:
                for img, inter in outs[k]:
                    top, left = (img.shape[2] - h) // 2, (img.shape[3] - w) // 2
                    v0 = inter[6][0, 0, top:top + h, left:left + w]
                    self.save((v0 * 255.0).clamp(0, 255).byte().cpu().numpy(), count, self.visibility_dir, "visibility")
                    np.save(os.path.join(self.flow_dir, "flow_t1_%05d.npy" % count),
                            inter[4][0, :, top:top + h, left:left + w].cpu().numpy())
                    np.save(os.path.join(self.flow_dir, "flow_t0_%05d.npy" % count),
                            inter[5][0, :, top:top + h, left:left + w].cpu().numpy())
                    if self.flow_png:          # refined flows per t (:168-182)
                        self.save_flow_png(inter[4], h, w, top, left, count, "refined_flow_t1", "flow_t1")
                        self.save_flow_png(inter[5], h, w, top, left, count, "refined_flow_t0", "flow_t0")
                    self.save(F.frames_to_u8(img, h, w, self.cfg)[0].cpu().numpy(), count, self.img_dir)
                    log.info("Interpolated frame: %s", count)
                    count += 1
                if self.flow_png and outs[k]:          # the pair's stage-1 flows, once, under the next original's number (:203-210)
                    inter = outs[k][-1][1]
                    top, left = (inter[0].shape[2] - h) // 2, (inter[0].shape[3] - w) // 2
                    self.save_flow_png(inter[0], h, w, top, left, count, "estimated_flow_01", "Flow_01")
                    self.save_flow_png(inter[1], h, w, top, left, count, "estimated_flow_10", "Flow_10")
                if self.consistency_png and outs[k]:          # beside the pair's stage-1 flow maps, under the same number
                    inter = outs[k][-1][1]
                    top, left = (inter[0].shape[2] - h) // 2, (inter[0].shape[3] - w) // 2
                    self.save_consistency_png(inter[0], inter[1], h, w, top, left, count)
            else:
                u8 = F.frames_to_u8(outs[k], h, w, self.cfg).cpu().numpy()
                for j in range(u8.shape[0]):
                    self.save(u8[j], count, self.img_dir)
                    log.info("Interpolated frame: %s", count)
                    count += 1
        self.save(frames_cpu[pos[windows[-1][1]]], count, self.img_dir)
        return count + 1


def main(argv=None, model=None):
    args = getargs(argv)
    config = configparser.RawConfigParser()
    logging.basicConfig(filename=args.log, level=logging.INFO)
    if not config.read(args.config):
        raise FileNotFoundError(args.config)
    n = Interpolator(config, args, model=model).interpolate_frames()
    log.info("Interpolation complete.")
    return n


if __name__ == "__main__":
    main()
