"""Training data: clip lists, index plans, frame sources and the loader that feeds Trainer.train from real clips.

  read_clip_list        the reference's list formats: ADOBE / NFS (scripts/utils/dataloaders/adobe_240fps.py:20-39, nfs.py), the VIMEO
                        septuplet lists (vimeo.py:25-46), DATASET = ALL = ADOBE + NFS + VIMEO (combined_dataset.py)
  window_plan /         which frames of a clip a sample reads and the time of its targets (default_reader.py:153-180, vimeo.py:79-115):
  vimeo_plan            pure functions of the drawn values
  read_frame_into       a frame, chosen by the path's extension: an image file through PIL, or frame k of a pre-decoded `.npy` clip
                        (`clip.npy#k`, written by scripts/utils/pack_clips.py) through a memory map; decoded uint8 goes straight into the
                        batch's pinned staging buffer - no float array is made on the host
  clip_batch_from_u8    the kernel (csrc/ssm_data.hip): staging buffer + record table -> the cropped, flipped, rotated, normalised
                        (input, target) tensors of the dataloader contract
  augment_host          numpy float32 yardstick that spells the kernel's operations in the kernel's order: the fixed point the kernel
                        is held to bit for bit (tests only)
  ClipLoader            the pipeline, in the shape of ssm_amd/video.py: decode threads fill a ring of pinned staging buffers, one H2D copy
                        and one kernel per batch run on the loader's stream behind an event, the consumer's stream waits for that event

Transform order of the reference: RandomCrop, then RandomMirrorRotate (shipped commented out there; `flip` / `rotate` opt in), then Normalize
and ToTensor (default_reader.py:250-286, augmentations.py:39-92,181-200).  Stated deviations: crop origins are drawn from [0, h - th] and
[0, w - tw] INCLUSIVE (the reference's randint(0, w - tw) never picks the last offset and throws when one side already fits); a list line
that is an integer is a frame count whatever its length (the reference tests len(line) <= 2, so a clip of 100 frames is lost); ADOBE and
NFS clips are windowed under DATASET = ALL too (the reference's test of the dataset name skips that); the rotation is the bilinear resampling
defined in include/ssm_hip.h, not cv2's fixed-point warpAffine.  Out of scope: the evaluation-mode readers, ResizeCrop, Binarize.
"""
import ctypes
import functools
import os
import queue
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from .frames import _f3, cfg_mean_std

INTERP_FACTOR = 8                                   # 240 fps clips, 30 fps inputs
REQD_IMAGES = {2: 9, 4: 25, 6: 41, 8: 57}           # frames of a window: 8 (N_FRAMES - 1) + 1
TRANSPOSE, HFLIP, AFFINE = 1, 2, 4                  # SSM_CLIP_* of include/ssm_hip.h
# ssm_clip_record of include/ssm_hip.h
RECORD = np.dtype([("offset", "<i8"), ("hs", "<i4"), ("ws", "<i4"), ("flags", "<i4"), ("y1", "<i4"), ("x1", "<i4"), ("a", "<f4", (6,)),
                   ("reserved", "<i4", (3,))])
assert RECORD.itemsize == 64
N_DRAWS = 9                                         # uniforms per sample: window start, reversal, s, y1, x1, flip, cx, cy, theta
_SECTIONS = {"ADOBE": "ADOBE_DATA", "NFS": "NFS_DATA", "VIMEO": "VIMEO_DATA"}


class ClipReadError(RuntimeError):
    """A frame could not be read or does not fit the batch; the message starts with its path."""


# ---- clip lists --------------------------------------------------------------------------------------------------------------------
def _is_int(line):
    return line.isdigit()


def parse_counted_list(lines):
    """ADOBE / NFS format: a line that is an integer n, then n frame paths.  An integer line directly followed by another one is the
    file's leading clip count (the reference's scripts/utils/make_clips.py writes one) and is skipped, as are stray lines between clips."""
    lines = [ln.strip() for ln in lines]
    clips, i = [], 0
    while i < len(lines):
        if _is_int(lines[i]):
            if i + 1 < len(lines) and _is_int(lines[i + 1]):
                i += 1
                continue
            n = int(lines[i])
            paths = lines[i + 1:i + 1 + n]
            if len(paths) != n or any(not p or _is_int(p) for p in paths):
                raise ValueError("clip list: line %d announces %d frames, %d paths follow" % (i + 1, n, len([p for p in paths if p and not _is_int(p)])))
            clips.append(paths)
            i += n + 1
        else:
            i += 1
    return clips


def read_clip_list(cfg, split="TRAIN", dataset=None):
    """[(kind, [frame paths])] of DATA.DATASET (or `dataset`): kind "window" for ADOBE / NFS clips (a random window is cut from them),
    "vimeo" for septuplets.  ALL concatenates ADOBE, NFS and VIMEO in that order."""
    name = dataset or cfg.get("DATA", "DATASET")
    if name == "ALL":
        return [c for d in ("ADOBE", "NFS", "VIMEO") for c in read_clip_list(cfg, split, d)]
    if name not in _SECTIONS:
        raise ValueError("DATA.DATASET = %s has no training reader (ADOBE, NFS, VIMEO and ALL have)" % name)
    sec = _SECTIONS[name]
    with open(cfg.get(sec, split + "PATHS")) as f:
        lines = f.readlines()
    if name == "VIMEO":
        root = cfg.get(sec, "ROOTDIR")
        return [("vimeo", [os.path.join(root, "sequences", s.strip()) + "/im%d.png" % i for i in range(1, 8)]) for s in lines if s.strip()]
    return [("window", c) for c in parse_counted_list(lines)]


def max_frame_bytes(cfg, dataset=None):
    """Bytes of the largest source frame: H_IN x W_IN x 3 of the sections DATA.DATASET reads."""
    name = dataset or cfg.get("DATA", "DATASET")
    names = ("ADOBE", "NFS", "VIMEO") if name == "ALL" else (name,)
    return max(cfg.getint(_SECTIONS[n], "H_IN") * cfg.getint(_SECTIONS[n], "W_IN") * 3 for n in names)


# ---- index plans -------------------------------------------------------------------------------------------------------------------
def reqd_images(n_frames):
    return REQD_IMAGES[n_frames]


def sample_s(t_sample, u):
    """The sampled position inside every window, from a uniform u in [0, 1): RANDOM 1..7, MIDDLE 4."""
    if t_sample == "RANDOM":
        return 1 + min(int(u * (INTERP_FACTOR - 1)), INTERP_FACTOR - 2)
    if t_sample == "MIDDLE":
        return INTERP_FACTOR // 2
    raise NotImplementedError("DATALOADER.T_SAMPLE = %s: training samples RANDOM or MIDDLE" % t_sample)


def window_plan(n_frames, s):
    """(input indexes, target indexes, t) inside a window of reqd_images(n_frames): inputs [0, 8, ..], one target s frames after every
    input but the last (the same s in all windows), t = s / 8."""
    if not 1 <= s <= INTERP_FACTOR - 1:
        raise ValueError("s = %d outside 1..7" % s)
    inputs = [i * INTERP_FACTOR for i in range(n_frames)]
    return inputs, [s + i * INTERP_FACTOR for i in range(n_frames - 1)], s / float(INTERP_FACTOR)


def vimeo_plan(n_frames, choice):
    """Septuplet rules (vimeo.py:79-115): `choice` in (1, 3, 5) is the interpolated frame; clip edges are replicated; t = 0.5."""
    if choice not in (1, 3, 5):
        raise ValueError("choice = %r not in (1, 3, 5)" % (choice,))
    if n_frames == 2:
        return [choice - 1, choice + 1], [choice], 0.5
    if n_frames == 4:
        return {1: ([0, 0, 2, 4], [0, 1, 3], 0.5), 3: ([0, 2, 4, 6], [1, 3, 5], 0.5), 5: ([2, 4, 6, 6], [3, 5, 6], 0.5)}[choice]
    raise ValueError("VIMEO supports N_FRAMES 2 or 4, not %d" % n_frames)


def _pick(u, n):
    """Uniform integer in [0, n) from u in [0, 1)."""
    return min(int(u * n), n - 1)


def rotation_inverse(cx, cy, theta_deg):
    """The six fp32 coefficients of the map from output to source pixels that cv2.warpAffine applies for M = cv2.getRotationMatrix2D((cx, cy),
    theta, 1): M = [[a, b, (1 - a) cx - b cy], [-b, a, b cx + (1 - a) cy]], a = cos, b = sin; inverted in float64, rounded once."""
    th = np.deg2rad(np.float64(theta_deg))
    a, b = np.cos(th), np.sin(th)
    m = np.array([[a, b, (1.0 - a) * cx - b * cy], [-b, a, b * cx + (1.0 - a) * cy]], dtype=np.float64)
    d = m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]
    i00, i01, i10, i11 = m[1, 1] / d, -m[0, 1] / d, -m[1, 0] / d, m[0, 0] / d
    inv = [i00, i01, -(i00 * m[0, 2] + i01 * m[1, 2]), i10, i11, -(i10 * m[0, 2] + i11 * m[1, 2])]
    return (np.array(inv, dtype=np.float64) + 0.0).astype(np.float32)          # (+ 0.0: no negative zeros)


class SamplePlan:
    """One sample of an epoch: the frames to read (inputs first, then targets), t of its targets and the draws that fix its record once
    the frame size is known."""
    __slots__ = ("index", "paths", "t", "uy", "ux", "hflip", "affine")

    def __init__(self, index, paths, t, uy, ux, hflip, affine):
        self.index, self.paths, self.t, self.uy, self.ux, self.hflip, self.affine = index, paths, t, uy, ux, hflip, affine

    def record(self, hs, ws, th, tw, offset=0):
        """The table record for stored frames of hs x ws: a stored frame with h > w is read transposed; the crop origin is uniform in
        [0, h - th] x [0, w - tw] inclusive."""
        transpose = hs > ws
        h, w = (ws, hs) if transpose else (hs, ws)
        if h < th or w < tw:
            raise ClipReadError("%s: a %dx%d frame is too small for the %dx%d crop" % (self.paths[0], h, w, th, tw))
        r = np.zeros((), dtype=RECORD)
        r["offset"], r["hs"], r["ws"] = offset, hs, ws
        r["y1"], r["x1"] = _pick(self.uy, h - th + 1), _pick(self.ux, w - tw + 1)
        r["flags"] = (TRANSPOSE if transpose else 0) | (HFLIP if self.hflip else 0) | (AFFINE if self.affine is not None else 0)
        if self.affine is not None:
            r["a"] = self.affine
        return r


def plan_sample(index, kind, paths, u, n_frames, t_sample, th, tw, flip=False, rotate=False):
    """SamplePlan of clip `index` from its N_DRAWS uniforms u, consumed in the order window start, reversal, s (VIMEO: the interpolated
    frame), y1, x1, flip, cx, cy, theta.  Every draw is consumed whether it is used or not, so no option moves another one's value."""
    if kind == "window":
        need = reqd_images(n_frames)
        if len(paths) < need:
            raise ClipReadError("%s: the clip has %d frames, N_FRAMES = %d needs %d" % (paths[0] if paths else "<empty clip>", len(paths), n_frames, need))
        start = _pick(u[0], len(paths) - need + 1)
        paths = paths[start:start + need]
    if u[1] >= 0.5:                                   # time reversal, probability 1/2 (default_reader.py:64-65)
        paths = paths[::-1]
    if kind == "window":
        inputs, targets, t = window_plan(n_frames, sample_s(t_sample, u[2]))
    else:
        inputs, targets, t = vimeo_plan(n_frames, (1, 3, 5)[_pick(u[2], 3)])
    affine = rotation_inverse(_pick(u[6], tw), _pick(u[7], th), -5.0 + 10.0 * u[8]) if rotate else None
    return SamplePlan(index, [paths[i] for i in inputs + targets], t, u[3], u[4], bool(flip and u[5] >= 0.5), affine)


def epoch_rng(seed, epoch):
    return np.random.Generator(np.random.PCG64([int(seed), int(epoch)]))


def shard(perm, batch, rank, world):
    """Sample i of the permutation goes to rank i mod world; whole batches only, the same number on every rank (an uneven count would
    hang the gradient all-reduce).  Returns the rank's batches as lists of positions in `perm`."""
    n_batches = len(perm) // (batch * world)
    mine = list(range(rank, n_batches * batch * world, world))
    return [mine[k * batch:(k + 1) * batch] for k in range(n_batches)]


# ---- frame sources -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=64)
def _open_npy(path):
    arr = np.load(path, mmap_mode="r")
    if arr.dtype != np.uint8 or arr.ndim != 4 or arr.shape[3] != 3:
        raise ValueError("expected a [T, H, W, 3] uint8 array, found %s %s" % (arr.dtype, arr.shape))
    return arr


def frame_source(path):
    """The stored frame behind `path` as an [H, W, 3] uint8 array(-like): `clip.npy#k` is frame k of a memory-mapped clip, anything else
    an image file decoded by PIL (which releases the GIL while decoding)."""
    try:
        base, sep, k = path.rpartition("#")
        if sep and base.endswith(".npy"):
            return _open_npy(base)[int(k)]
        from PIL import Image
        with Image.open(path) as im:
            return np.asarray(im.convert("RGB"))
    except ClipReadError:
        raise
    except Exception as e:          # noqa: BLE001 - every reader error names its file
        raise ClipReadError("%s: %s: %s" % (path, type(e).__name__, e)) from e


def read_frame_into(path, buf, base, k, limit):
    """Copy the stored frame behind `path` into the flat uint8 buffer `buf` as frame k of the sample that starts at byte `base`: behind
    its k predecessors, whose size it shares (the caller checks that).  `limit`: the bytes a frame may take.  Returns (H, W)."""
    arr = frame_source(path)
    h, w = int(arr.shape[0]), int(arr.shape[1])
    n = h * w * 3
    if n > limit:
        raise ClipReadError("%s: a %dx%d frame is larger than the configured H_IN x W_IN (%d bytes)" % (path, h, w, limit))
    np.copyto(buf[base + k * n:base + (k + 1) * n].reshape(h, w, 3), arr)
    return h, w


def logical_frames(frames_u8):
    """[F, Hs, Ws, 3] stored frames -> the frames the transform sees: transposed when stored with h > w (default_reader.py:203-205)."""
    return frames_u8.swapaxes(1, 2) if frames_u8.shape[1] > frames_u8.shape[2] else frames_u8


# ---- yardstick ---------------------------------------------------------------------------------------------------------------------
_F = np.float32


def augment_host(frames_u8, record, mean, std, crop=None):
    """Yardstick of ssm_clip_batch_from_u8_fwd for one sample: [F, Hs, Ws, 3] uint8 stored frames + its record -> [F, 3, th, tw] float32,
    every operation one rounded fp32 operation in the kernel's order (include/ssm_hip.h).  crop = (th, tw); default: everything from
    the origin to the frame's end."""
    frames_u8 = np.asarray(frames_u8)
    flags = int(record["flags"])
    lf = frames_u8.swapaxes(1, 2) if flags & TRANSPOSE else frames_u8
    y1, x1 = int(record["y1"]), int(record["x1"])
    th, tw = crop if crop is not None else (lf.shape[1] - y1, lf.shape[2] - x1)
    c = lf[:, y1:y1 + th, x1:x1 + tw]
    assert c.shape[1:3] == (th, tw), "the crop leaves the frame"
    if flags & HFLIP:
        c = c[:, :, ::-1]
    s = c.astype(_F)                                   # [F, th, tw, 3]
    if flags & AFFINE:
        a = np.asarray(record["a"], dtype=_F)
        x, y = np.arange(tw, dtype=_F)[None, :], np.arange(th, dtype=_F)[:, None]
        u = (a[0] * x + a[1] * y) + a[2]
        v = (a[3] * x + a[4] * y) + a[5]
        with np.errstate(invalid="ignore"):
            ok = (u > -1) & (u < tw) & (v > -1) & (v < th)
        u, v = np.where(ok, u, _F(0)), np.where(ok, v, _F(0))
        uf, vf = np.floor(u), np.floor(v)
        i, j = uf.astype(np.int64), vf.astype(np.int64)
        ax, ay = u - uf, v - vf
        bx, by = _F(1) - ax, _F(1) - ay
        pad = np.zeros((s.shape[0], th + 2, tw + 2, 3), dtype=_F)          # the constant border: taps at -1 and at th / tw read 0
        pad[:, 1:-1, 1:-1] = s

        def tap(dy, dx):
            return pad[:, j + 1 + dy, i + 1 + dx]

        ax, ay, bx, by = ax[None, :, :, None], ay[None, :, :, None], bx[None, :, :, None], by[None, :, :, None]
        top = tap(0, 0) * bx + tap(0, 1) * ax
        bot = tap(1, 0) * bx + tap(1, 1) * ax
        s = np.where(ok[None, :, :, None], top * by + bot * ay, _F(0))
    m, sd = np.asarray(mean, dtype=_F), np.asarray(std, dtype=_F)
    out = (s / _F(255.0) - m) / sd
    return np.ascontiguousarray(out.transpose(0, 3, 1, 2))


# ---- the kernel --------------------------------------------------------------------------------------------------------------------
def clip_batch_from_u8(staging, table, inputs, targets, cfg=None):
    """staging: flat uint8 device tensor that starts with the B records of `table` (a host numpy array of RECORD, offsets in bytes from
    the start of `staging`); inputs [B, n_in, 3, th, tw], targets [B, F - n_in, 3, th, tw]: contiguous fp32 device tensors to fill."""
    import torch

    from . import hipbind as hb
    assert staging.is_cuda and staging.dtype == torch.uint8 and staging.dim() == 1 and staging.is_contiguous(), "staging: flat uint8 on the GPU"
    for t in (inputs, targets):
        hb.require_device(t, "batch tensor")
        assert t.dim() == 5 and t.is_contiguous() and t.shape[2] == 3
    table = np.ascontiguousarray(table, dtype=RECORD)
    b, n_in, _, th, tw = inputs.shape
    assert targets.shape[0] == b and tuple(targets.shape[3:]) == (th, tw) and table.shape == (b,)
    mean, std = cfg_mean_std(cfg)
    hb.check(hb.load().ssm_clip_batch_from_u8_fwd(staging.data_ptr(), staging.numel(), staging.data_ptr(), table.ctypes.data_as(ctypes.c_void_p),
                                                  inputs.data_ptr(), targets.data_ptr(), b, n_in + targets.shape[1], n_in, th, tw, _f3(mean),
                                                  _f3(std), hb.stream_ptr()))


# ---- the loader --------------------------------------------------------------------------------------------------------------------
def worker_count(cfg, n_workers=None):
    """Decode threads: DATALOADER.N_WORKERS, at most the CPUs this process may run on and 16 (never sized from os.cpu_count())."""
    n = cfg.getint("DATALOADER", "N_WORKERS") if n_workers is None else int(n_workers)
    return max(1, min(n, len(os.sched_getaffinity(0)), 16))


def _align(n, a=256):
    return (n + a - 1) // a * a


class ClipLoader:
    """An iterable of (input [B,N,3,th,tw], target [B,N-1,3,th,tw], t_interp [B,N-1,1,1,1]) device batches of one epoch; iterate it
    once per epoch (set_epoch, or let every iteration advance the epoch).

    Randomness: every draw of an epoch is made on the consumer's thread when the iteration starts, from
    numpy.random.Generator(PCG64([seed, epoch])): the permutation of the clips, then N_DRAWS uniforms per sample in sample order.  A batch
    depends on (seed, epoch, rank, world) and the data only, never on the thread count or on timing.
    Pipeline: a ring of `depth` slots, each a pinned staging buffer (record table, t, then a fixed room per sample), its device copy and
    its two output tensors.  A feeder thread takes a free slot, has the decode threads (a ThreadPoolExecutor: threads, never processes - a
    process that has initialised HIP must not fork) copy the frames into it, writes the table, and queues one H2D copy and the kernel on
    the loader's stream, with an event behind them; the consumer's stream waits for that event.  The tensors of a batch stay valid until
    the consumer asks for the next one: an event recorded on the consumer's stream at that moment gates the slot's reuse.  Host and device
    memory are fixed by depth, B, F and the largest source frame (H_IN x W_IN of the ini).
    Failures: an unreadable or unfit frame ends the epoch with a ClipReadError naming the path in the consumer; pending work is cancelled
    and the threads are joined."""

    def __init__(self, cfg, split, device, rank=0, world=1, seed=0, n_workers=None, depth=3, flip=False, rotate=False):
        self.cfg, self.split, self.device = cfg, split, device
        self.rank, self.world, self.seed = int(rank), int(world), int(seed)
        assert 0 <= self.rank < self.world
        self.n_workers, self.depth = worker_count(cfg, n_workers), max(2, int(depth))
        self.flip, self.rotate = bool(flip), bool(rotate)
        self.n_frames = cfg.getint("TRAIN", "N_FRAMES")
        self.F = 2 * self.n_frames - 1
        self.batch = cfg.getint(split, "BATCH_SIZE")
        self.th, self.tw = cfg.getint(split, "CROP_IMH"), cfg.getint(split, "CROP_IMW")
        self.t_sample = cfg.get("DATALOADER", "T_SAMPLE")
        self.clips = read_clip_list(cfg, split)
        if any(k == "window" for k, _ in self.clips):
            sample_s(self.t_sample, 0.0)               # a T_SAMPLE that cannot train is refused here, not in the middle of an epoch
        self.frame_room = max_frame_bytes(cfg)
        self.sample_room = _align(self.F * self.frame_room)
        self.t_offset = _align(self.batch * RECORD.itemsize)
        self.head = _align(self.t_offset + 4 * self.batch * (self.n_frames - 1))
        self.staging_bytes = self.head + self.batch * self.sample_room
        self.epoch = 0
        self._slots = None

    def __len__(self):
        return len(self.clips) // (self.batch * self.world)

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    # -- planning (host only) --
    def plan_epoch(self, epoch=None):
        """The rank's batches of an epoch as lists of SamplePlan."""
        rng = epoch_rng(self.seed, self.epoch if epoch is None else epoch)
        perm = rng.permutation(len(self.clips))
        draws = rng.random((len(self.clips), N_DRAWS))
        out = []
        for pos in shard(perm, self.batch, self.rank, self.world):
            out.append([plan_sample(int(perm[p]), self.clips[perm[p]][0], self.clips[perm[p]][1], draws[p], self.n_frames, self.t_sample,
                                    self.th, self.tw, self.flip, self.rotate) for p in pos])
        return out

    def fill(self, buf, plans, pool):
        """Decode one batch into the staging buffer `buf` (flat uint8 numpy, staging_bytes long) on `pool`; writes the table and t at its
        head.  Returns (table, bytes used)."""
        futs = []
        try:
            for b, sp in enumerate(plans):
                base = self.head + b * self.sample_room
                for k, path in enumerate(sp.paths):
                    futs.append(pool.submit(read_frame_into, path, buf, base, k, self.frame_room))
            sizes = [f.result() for f in futs]
        except BaseException:
            for f in futs:
                f.cancel()
            raise
        table = np.zeros(len(plans), dtype=RECORD)
        used = self.head
        for b, sp in enumerate(plans):
            mine = sizes[b * self.F:(b + 1) * self.F]
            for k, sz in enumerate(mine):
                if sz != mine[0]:
                    raise ClipReadError("%s: a %dx%d frame in a clip of %dx%d frames" % (sp.paths[k], sz[0], sz[1], mine[0][0], mine[0][1]))
            table[b] = sp.record(mine[0][0], mine[0][1], self.th, self.tw, self.head + b * self.sample_room)
            used = self.head + b * self.sample_room + self.F * mine[0][0] * mine[0][1] * 3
        buf[:table.nbytes] = table.view(np.uint8)
        t = np.array([[sp.t] * (self.n_frames - 1) for sp in plans], dtype=np.float32)
        buf[self.t_offset:self.t_offset + t.nbytes] = t.reshape(-1).view(np.uint8)
        return table, _align(used, 4)

    def host_batches(self, epoch=None, n_workers=None):
        """The host half alone, for tests and tools: yields (plans, table, [stored frames [F,Hs,Ws,3] uint8 per sample], t [B,N-1]) per batch."""
        buf = np.zeros(self.staging_bytes, dtype=np.uint8)
        with ThreadPoolExecutor(self.n_workers if n_workers is None else n_workers, thread_name_prefix="clip-loader-w") as pool:
            for plans in self.plan_epoch(epoch):
                table, _ = self.fill(buf, plans, pool)
                frames = [buf[r["offset"]:r["offset"] + self.F * r["hs"] * r["ws"] * 3].reshape(self.F, r["hs"], r["ws"], 3).copy() for r in table]
                t = buf[self.t_offset:self.t_offset + 4 * len(plans) * (self.n_frames - 1)].view(np.float32).reshape(len(plans), -1).copy()
                yield plans, table, frames, t

    def yardstick(self, table, frames):
        """[B,N,3,th,tw], [B,N-1,3,th,tw] float32 numpy: augment_host of every sample (tests)."""
        mean, std = cfg_mean_std(self.cfg)
        x = np.stack([augment_host(f, r, mean, std, (self.th, self.tw)) for f, r in zip(frames, table)])
        return x[:, :self.n_frames], x[:, self.n_frames:]

    # -- the device pipeline --
    def _allocate(self):
        import torch
        dev, b, n = self.device, self.batch, self.n_frames
        slots = []
        for _ in range(self.depth):
            pinned = torch.empty(self.staging_bytes, dtype=torch.uint8).pin_memory()
            staging = torch.empty(self.staging_bytes, dtype=torch.uint8, device=dev)
            t = staging[self.t_offset:self.t_offset + 4 * b * (n - 1)].view(torch.float32).view(b, n - 1, 1, 1, 1)
            slots.append({"pinned": pinned, "np": pinned.numpy(), "staging": staging, "t": t,
                          "input": torch.empty(b, n, 3, self.th, self.tw, dtype=torch.float32, device=dev),
                          "target": torch.empty(b, n - 1, 3, self.th, self.tw, dtype=torch.float32, device=dev),
                          "ready": torch.cuda.Event(), "released": torch.cuda.Event()})
        self._slots, self._stream = slots, torch.cuda.Stream(device=dev)

    def __iter__(self):
        import torch
        epoch = self.epoch
        self.epoch += 1
        batches = self.plan_epoch(epoch)               # every draw of the epoch: here, on the consumer's thread
        if not batches:
            return
        if self._slots is None:
            self._allocate()
        slots, dev = self._slots, self.device
        self._stream.wait_stream(torch.cuda.current_stream(dev))          # the last epoch's batches may still be read: slots start free behind that
        free, ready, stop = queue.Queue(), queue.Queue(), threading.Event()
        for i in range(self.depth):
            free.put((i, None))
        pool = ThreadPoolExecutor(self.n_workers, thread_name_prefix="clip-loader-w")

        def feed():
            try:
                torch.cuda.set_device(dev)
                for plans in batches:
                    i, released = free.get()
                    if stop.is_set() or i is None:
                        return
                    if released is not None:
                        released.synchronize()          # the consumer is done with the slot's tensors (and the H2D before them with its pinned buffer)
                    s = slots[i]
                    table, used = self.fill(s["np"], plans, pool)
                    if stop.is_set():
                        return
                    with torch.cuda.stream(self._stream):
                        s["staging"][:used].copy_(s["pinned"][:used], non_blocking=True)
                        clip_batch_from_u8(s["staging"], table, s["input"], s["target"], self.cfg)
                        s["ready"].record()
                    ready.put((i, None))
                ready.put((None, None))
            except BaseException as e:          # noqa: BLE001 - handed to the consumer's thread
                ready.put((None, e))

        th = threading.Thread(target=feed, name="clip-loader-feed", daemon=True)
        th.start()
        held = None
        try:
            while True:
                if held is not None:                   # the consumer asks for the next batch: its work on the last one is queued by now
                    slots[held]["released"].record(torch.cuda.current_stream(dev))
                    free.put((held, slots[held]["released"]))
                    held = None
                i, err = ready.get()
                if err is not None:
                    raise err
                if i is None:
                    return
                s = slots[i]
                torch.cuda.current_stream(dev).wait_event(s["ready"])
                held = i
                yield s["input"], s["target"], s["t"]
        finally:
            stop.set()
            free.put((None, None))
            pool.shutdown(wait=True, cancel_futures=True)
            th.join()
            self._stream.synchronize()
