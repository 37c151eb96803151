"""Streamed slow-motion video: YUV4MPEG2 in, YUV4MPEG2 out, colour conversion on the GPU.

  Y4MReader / Y4MWriter   the one video container that needs no codec (every player and ffmpeg read and write it, pipes included):
                          a text header `YUV4MPEG2 W H F I A C X...`, then `FRAME` records of 8-bit planar Y, U, V
  yuv_table               the conversion constants, float64 rounded once to fp32: what csrc/ssm_video.hip and the yardsticks both read
  yuv_to_frames_host /    numpy float32 yardsticks that spell the two kernels' operations in the kernels' order: the fixed points the
  frames_to_yuv_host      kernels are held to bit for bit (as scripts/utils/flo_utils.py is for csrc/ssm_flow.hip)
  frames_from_yuv /       the kernels: payloads on the device <-> the path's normalised, padded fp32 planes, in the visualiser's
  frames_to_yuv           convention (scripts/visualize_interpolation.py:61-88,223-268)
  VideoInterpolator       the streamed loop: every leg of a pass (H2D, ingest, the pair pipeline, egress, D2H) is queued on the pass's HIP
                          stream, a writer thread drains a ring of pinned buffers in order; memory does not depend on the clip's length

Out of scope: codecs, audio, more than 8 bits per sample, the recurrent configuration (N_FRAMES > 2).
"""
import ctypes
import queue
import sys
import threading

import numpy as np
import torch

from . import hipbind as hb
from .frames import _f3, cfg_mean_std, padded_dims

BT601, BT709 = 0, 1
LIMITED, FULL = 0, 1
CENTRED, COSITED, C444 = 0, 1, 2          # chroma siting (include/ssm_hip.h SSM_YUV_*)
YUV_ROW = 20
MATRICES = {"bt601": BT601, "bt709": BT709}
RANGES = {"limited": LIMITED, "full": FULL}
# Y4M colour-space tags: accepted -> siting; refused ones are named in the error
CHROMA_TAGS = {"420": CENTRED, "420jpeg": CENTRED, "420mpeg2": COSITED, "444": C444}
_KRKB = {BT601: (0.299, 0.114), BT709: (0.2126, 0.0722)}


def yuv_table():
    """[2 matrices][2 ranges][YUV_ROW] float32: every constant evaluated in float64 and rounded once (layout: include/ssm_hip.h)."""
    t = np.zeros((2, 2, YUV_ROW), dtype=np.float64)
    for m, (kr, kb) in _KRKB.items():
        kg = 1.0 - kr - kb
        for r in (LIMITED, FULL):
            lim = r == LIMITED
            t[m, r, :19] = [kr, kg, kb,
                            2.0 * (1.0 - kr), 2.0 * (1.0 - kb) * kb / kg, 2.0 * (1.0 - kr) * kr / kg, 2.0 * (1.0 - kb),
                            1.0 / (2.0 * (1.0 - kb)), 1.0 / (2.0 * (1.0 - kr)),
                            255.0 / 219.0 if lim else 1.0, 255.0 / 224.0 if lim else 1.0,
                            219.0 / 255.0 if lim else 1.0, 224.0 / 255.0 if lim else 1.0,
                            16.0 if lim else 0.0, 128.0,
                            16.0 if lim else 0.0, 235.0 if lim else 255.0, 16.0 if lim else 0.0, 240.0 if lim else 255.0]
    return t.astype(np.float32)


_table_c = None


def _table_ptr():
    global _table_c
    if _table_c is None:
        flat = yuv_table().reshape(-1)
        _table_c = (ctypes.c_float * flat.size)(*[float(v) for v in flat])
    return _table_c


def chroma_dims(h, w, siting):
    return (h, w) if siting == C444 else ((h + 1) // 2, (w + 1) // 2)


def frame_bytes(h, w, siting):
    ch, cw = chroma_dims(h, w, siting)
    return h * w + 2 * ch * cw


def split_planes(payload, h, w, siting):
    """[N, frame_bytes] uint8 -> Y [N,h,w], U, V [N,ch,cw] (views)."""
    ch, cw = chroma_dims(h, w, siting)
    n = payload.shape[0]
    y = payload[:, :h * w].reshape(n, h, w)
    u = payload[:, h * w:h * w + ch * cw].reshape(n, ch, cw)
    v = payload[:, h * w + ch * cw:].reshape(n, ch, cw)
    return y, u, v


def default_matrix(h):
    """BT.709 for HD (720 rows and up), BT.601 below: what players assume of untagged material."""
    return BT709 if h >= 720 else BT601


# ---- numpy float32 yardsticks: the kernels' operations in the kernels' order -------------------------------------------------------
_F = np.float32


def _upsample_host(c, h, w, siting):
    """Chroma plane [N,ch,cw] float32 -> [N,h,w]: bilinear, indices clamped; columns first, then rows, as the kernel."""
    ch, cw = c.shape[1:]
    x = np.arange(w)
    j, odd = x // 2, (x % 2) == 1
    a0, a1, b1, b2 = (_F(0.0), _F(1.0), _F(0.5), _F(0.5)) if siting == COSITED else (_F(0.25), _F(0.75), _F(0.75), _F(0.25))
    ia = np.clip(np.where(odd, j, j - 1), 0, cw - 1)
    ib = np.clip(np.where(odd, j + 1, j), 0, cw - 1)
    wa = np.where(odd, b1, a0).astype(_F)
    wb = np.where(odd, b2, a1).astype(_F)
    hz = wa * c[:, :, ia] + wb * c[:, :, ib]
    y = np.arange(h)
    i, odd = y // 2, (y % 2) == 1
    ia = np.clip(np.where(odd, i, i - 1), 0, ch - 1)
    ib = np.clip(np.where(odd, i + 1, i), 0, ch - 1)
    wa = np.where(odd, _F(0.75), _F(0.25)).astype(_F)[None, :, None]
    wb = np.where(odd, _F(0.25), _F(0.75)).astype(_F)[None, :, None]
    return wa * hz[:, ia] + wb * hz[:, ib]


def yuv_to_frames_host(payload, h, w, siting=CENTRED, matrix=BT709, color_range=LIMITED, mean=None, std=None, pad_before_norm=True):
    """Yardstick of ssm_frames_from_yuv_fwd: [N, frame_bytes] uint8 (numpy) -> [N,3,Hp,Wp] float32."""
    if mean is None:
        mean, std = cfg_mean_std(None)
    k = yuv_table()[matrix, color_range]
    kr, kg, kb, rv, gu, gv, bu, cbs, crs, ys, cs, iys, ics, yoff, coff = k[:15]
    payload = np.ascontiguousarray(payload).reshape(-1, frame_bytes(h, w, siting))
    yq, uq, vq = split_planes(payload, h, w, siting)
    yl, cu, cv = yq.astype(_F), uq.astype(_F), vq.astype(_F)
    if siting != C444:
        cu, cv = _upsample_host(cu, h, w, siting), _upsample_host(cv, h, w, siting)
    yl = (yl - yoff) * ys
    cb = (cu - coff) * cs
    cr = (cv - coff) * cs
    rgb = (yl + rv * cr, (yl - gu * cb) - gv * cr, yl + bu * cb)
    (hp, wp), (top, left) = padded_dims(h, w)
    out = np.zeros((payload.shape[0], 3, hp, wp), dtype=_F)
    for p in range(3):
        m, s = _F(mean[p]), _F(std[p])
        if pad_before_norm:
            out[:, p] = (_F(0.0) / _F(255.0) - m) / s
        out[:, p, top:top + h, left:left + w] = (np.clip(rgb[p], _F(0.0), _F(255.0)) / _F(255.0) - m) / s
    return out


def frames_to_yuv_host(x, h, w, siting=CENTRED, matrix=BT709, color_range=LIMITED, mean=None, std=None):
    """Yardstick of ssm_frames_to_yuv_fwd: [N,3,Hp,Wp] float32 (numpy, finite) -> [N, frame_bytes] uint8."""
    if mean is None:
        mean, std = cfg_mean_std(None)
    k = yuv_table()[matrix, color_range]
    kr, kg, kb, rv, gu, gv, bu, cbs, crs, ys, cs, iys, ics, yoff, coff, ylo, yhi, clo, chi = k[:19]
    x = np.asarray(x, dtype=_F)
    n, _, hp, wp = x.shape
    top, left = (hp - h) // 2, (wp - w) // 2
    rgb = []
    for p in range(3):
        v = x[:, p, top:top + h, left:left + w] * _F(std[p]) + _F(mean[p])
        rgb.append(v * _F(255.0))
    r, g, b = rgb
    yf = (kr * r + kg * g) + kb * b
    cb = (b - yf) * cbs
    cr = (r - yf) * crs

    def sub(c):
        if siting == C444:
            return c
        ch, cw = chroma_dims(h, w, siting)
        cx, cy = np.arange(cw), np.arange(ch)
        c0, c1 = 2 * cx, np.minimum(2 * cx + 1, w - 1)
        r0, r1 = 2 * cy, np.minimum(2 * cy + 1, h - 1)
        if siting == COSITED:
            cl = np.maximum(2 * cx - 1, 0)
            hz = ((c[:, :, cl] + _F(2.0) * c[:, :, c0]) + c[:, :, c1]) * _F(0.25)
            return (hz[:, r0] + hz[:, r1]) * _F(0.5)
        t, bt = c[:, r0], c[:, r1]
        return ((t[:, :, c0] + t[:, :, c1]) + (bt[:, :, c0] + bt[:, :, c1])) * _F(0.25)

    def code(v, scale, off, lo, hi):
        return np.clip(np.rint(v * scale + off), lo, hi).astype(np.uint8)

    planes = [code(yf, iys, yoff, ylo, yhi), code(sub(cb), ics, coff, clo, chi), code(sub(cr), ics, coff, clo, chi)]
    return np.concatenate([p.reshape(n, -1) for p in planes], axis=1)


# ---- the kernels -------------------------------------------------------------------------------------------------------------------
def frames_from_yuv(payload, h, w, siting=CENTRED, matrix=BT709, color_range=LIMITED, cfg=None, pad_before_norm=True, out=None, multiple=32):
    """[N, frame_bytes] uint8 device tensor of Y4M payloads -> [N,3,Hp,Wp] normalised fp32 (into `out` if given); (Hp, Wp) =
    padded_dims(h, w, multiple): 32 for the path itself, 32 * flow_scale for the coarse-flow mode."""
    assert payload.is_cuda and payload.dtype == torch.uint8 and payload.dim() == 2 and payload.is_contiguous() and \
        payload.shape[1] == frame_bytes(h, w, siting), "payloads must be a contiguous [N, frame_bytes] uint8 tensor on the GPU"
    n = payload.shape[0]
    (hp, wp), (top, left) = padded_dims(h, w, multiple)
    mean, std = cfg_mean_std(cfg)
    if out is None:
        out = torch.empty(n, 3, hp, wp, dtype=torch.float32, device=payload.device)
    assert tuple(out.shape) == (n, 3, hp, wp)
    hb.check(hb.load().ssm_frames_from_yuv_fwd(payload.data_ptr(), hb.view_of(out), n, h, w, hp, wp, top, left, _f3(mean), _f3(std),
                                               1 if pad_before_norm else 0, _table_ptr(), matrix, color_range, siting, hb.stream_ptr()))
    return out


def frames_to_yuv(x, h, w, siting=CENTRED, matrix=BT709, color_range=LIMITED, cfg=None, out=None):
    """[N,3,Hp,Wp] normalised fp32 (finite) -> [N, frame_bytes] uint8 payloads, the centred padding cropped away."""
    hb.require_device(x, "frame tensor")
    n, _, hp, wp = x.shape
    top, left = (hp - h) // 2, (wp - w) // 2
    mean, std = cfg_mean_std(cfg)
    if out is None:
        out = torch.empty(n, frame_bytes(h, w, siting), dtype=torch.uint8, device=x.device)
    assert out.is_contiguous() and tuple(out.shape) == (n, frame_bytes(h, w, siting)) and out.dtype == torch.uint8
    hb.check(hb.load().ssm_frames_to_yuv_fwd(hb.view_of(x), out.data_ptr(), n, h, w, top, left, _f3(mean), _f3(std), _table_ptr(),
                                             matrix, color_range, siting, hb.stream_ptr()))
    return out


# ---- YUV4MPEG2 ---------------------------------------------------------------------------------------------------------------------
class Y4MError(ValueError):
    pass


def _ratio(text, what):
    try:
        a, b = text.split(":")
        return int(a), int(b)
    except ValueError:
        raise Y4MError("bad %s %r in the Y4M header" % (what, text)) from None


class Y4MReader:
    """A YUV4MPEG2 stream from a path, `-` (stdin) or a binary file object.  Attributes: width, height, rate (num, den), interlace,
    aspect (num, den), chroma (the C tag's text, `420jpeg` when absent), siting, color_range (LIMITED / FULL from ffmpeg's
    XCOLORRANGE tag, None when absent), xtags (every X tag as read), frame_bytes."""

    def __init__(self, src):
        self._own = isinstance(src, str) and src != "-"
        self.f = open(src, "rb") if self._own else (sys.stdin.buffer if src == "-" else src)
        line = self.f.readline(4096)
        if not line.endswith(b"\n") or not line.startswith(b"YUV4MPEG2"):
            raise Y4MError("not a YUV4MPEG2 stream (no `YUV4MPEG2 ...` header line)")
        toks = line[:-1].decode("ascii", "replace").split(" ")
        if toks[0] != "YUV4MPEG2":
            raise Y4MError("not a YUV4MPEG2 stream (signature %r)" % toks[0])
        self.width = self.height = None
        self.rate, self.aspect, self.interlace, self.chroma, self.xtags = (25, 1), (0, 0), "p", "420jpeg", []
        for t in toks[1:]:
            if not t:
                continue
            key, val = t[0], t[1:]
            if key == "W":
                self.width = int(val)
            elif key == "H":
                self.height = int(val)
            elif key == "F":
                self.rate = _ratio(val, "frame rate")
            elif key == "A":
                self.aspect = _ratio(val, "pixel aspect")
            elif key == "I":
                self.interlace = val
            elif key == "C":
                self.chroma = val
            elif key == "X":
                self.xtags.append(val)
            else:
                raise Y4MError("unknown Y4M header field %r" % t)
        if not self.width or not self.height or self.width < 1 or self.height < 1:
            raise Y4MError("the Y4M header has no frame size (W, H)")
        if self.interlace not in ("p", "?"):
            raise Y4MError("interlaced Y4M input (I%s) is not supported: deinterlace first" % self.interlace)
        if self.chroma not in CHROMA_TAGS:
            raise Y4MError("Y4M colour space C%s is not supported (8-bit C420, C420jpeg, C420mpeg2 and C444 are)" % self.chroma)
        self.siting = CHROMA_TAGS[self.chroma]
        self.color_range = None
        for x in self.xtags:
            if x.startswith("COLORRANGE="):
                v = x.split("=", 1)[1].lower()
                if v not in RANGES:
                    raise Y4MError("unknown XCOLORRANGE=%s in the Y4M header" % x.split("=", 1)[1])
                self.color_range = RANGES[v]
        self.frame_bytes = frame_bytes(self.height, self.width, self.siting)
        self.frames_read = 0

    def read_frame_into(self, buf):
        """The next frame's payload into `buf` (writable, frame_bytes long; e.g. a row of a pinned tensor as numpy).  False at the end of
        the stream; a record cut short is an error, not the end."""
        line = self.f.readline(4096)
        if not line:
            return False
        if not line.endswith(b"\n") or not (line == b"FRAME\n" or line.startswith(b"FRAME ")):
            raise Y4MError("frame %d: expected a FRAME record, got %r" % (self.frames_read, line[:16]))
        mv = memoryview(buf).cast("B")
        if len(mv) != self.frame_bytes:
            raise ValueError("buffer of %d bytes for frames of %d" % (len(mv), self.frame_bytes))
        got = 0
        while got < len(mv):
            n = self.f.readinto(mv[got:])
            if not n:
                raise Y4MError("frame %d is truncated: %d of %d bytes" % (self.frames_read, got, len(mv)))
            got += n
        self.frames_read += 1
        return True

    def close(self):
        if self._own:
            self.f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class Y4MWriter:
    """Writes the stream header at once, then one FRAME record per write_frame()."""

    def __init__(self, dst, width, height, rate=(25, 1), aspect=(0, 0), chroma="420jpeg", color_range=None, interlace="p", xtags=()):
        if chroma not in CHROMA_TAGS:
            raise Y4MError("Y4M colour space C%s is not supported (8-bit C420, C420jpeg, C420mpeg2 and C444 are)" % chroma)
        self._own = isinstance(dst, str) and dst != "-"
        self.f = open(dst, "wb") if self._own else (sys.stdout.buffer if dst == "-" else dst)
        self.width, self.height, self.rate, self.aspect, self.chroma = int(width), int(height), tuple(rate), tuple(aspect), chroma
        self.siting, self.color_range, self.interlace = CHROMA_TAGS[chroma], color_range, interlace
        self.xtags = [x for x in xtags if not x.startswith("COLORRANGE=")]
        if color_range is not None:
            self.xtags.append("COLORRANGE=" + ("FULL" if color_range == FULL else "LIMITED"))
        self.frame_bytes = frame_bytes(self.height, self.width, self.siting)
        self.frames_written = 0
        head = "YUV4MPEG2 W%d H%d F%d:%d I%s A%d:%d C%s" % (self.width, self.height, self.rate[0], self.rate[1], interlace,
                                                            self.aspect[0], self.aspect[1], chroma)
        self.f.write((head + "".join(" X" + x for x in self.xtags) + "\n").encode("ascii"))

    @classmethod
    def like(cls, dst, reader, rate=None, color_range=None):
        """A writer for frames of `reader`'s format; `rate` and `color_range` override the reader's."""
        return cls(dst, reader.width, reader.height, rate or reader.rate, reader.aspect, reader.chroma,
                   reader.color_range if color_range is None else color_range, "p", reader.xtags)

    def write_frame(self, buf):
        mv = memoryview(buf).cast("B")
        if len(mv) != self.frame_bytes:
            raise ValueError("frame of %d bytes, the stream's frames have %d" % (len(mv), self.frame_bytes))
        self.f.write(b"FRAME\n")
        self.f.write(mv)
        self.frames_written += 1

    def close(self):
        self.f.flush()
        if self._own:
            self.f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


# ---- output order -------------------------------------------------------------------------------------------------------------------
def pass_order(valid, nt):
    """Write order of one pass of `valid` pairs with nt interpolated frames each: ("interp", row of the pass's output buffer) for the
    frames between a pair, then ("orig", row of the pass's input buffer) for the pair's right frame, its own input bytes."""
    for p in range(valid):
        for i in range(nt):
            yield "interp", p * nt + i
        yield "orig", p


def clip_order(n_frames, rate, pairs_per_batch=1):
    """The output of an n-frame clip as (input frame index, step): step 0 is input frame `index` itself, step s in 1..rate-1 the frame
    at t = s / rate between inputs `index` and `index + 1`.  (n - 1) * rate + 1 entries; composed of pass_order as run() composes it."""
    out = [(0, 0)] if n_frames > 0 else []
    nt, done = rate - 1, 0
    while done < n_frames - 1:
        valid = min(pairs_per_batch, n_frames - 1 - done)
        for kind, row in pass_order(valid, nt):
            out.append((done + row // nt, row % nt + 1) if kind == "interp" else (done + row + 1, 0))
        done += valid
    return out


def output_rate(rate, upsample_rate, slowmo=False):
    """Frame rate (num, den) of the output header: the input's times upsample_rate (same duration), or with slowmo the input's."""
    return (rate[0], rate[1]) if slowmo else (rate[0] * int(upsample_rate), rate[1])


# ---- the streamed loop -------------------------------------------------------------------------------------------------------------
class VideoInterpolator:
    """reader -> (upsample_rate - 1) frames between every two input frames -> writer, streamed.

    A pass takes `pairs_per_batch` new frames: H2D of their payloads, ingest (each frame once: its planes are the right frame of one
    pair and, carried over, the left frame of the next), the PairPipeline engine of the pass's stream, egress, D2H into the pass's slot
    of a ring of pinned buffers - all queued on that stream, nothing synchronises the host inside the loop but the ring itself.  A
    writer thread waits for a slot's event and writes, per pair, the interpolated frames and then the right frame's own input bytes.
    Host and device memory are fixed by the frame size, n_streams and pairs_per_batch."""

    def __init__(self, model, cfg, upsample_rate=8, n_streams=2, pairs_per_batch=1, matrix=None, color_range=None, flow_scale=1,
                 tile=None, halo=256, blend=32):
        """flow_scale = 2 or 4: the coarse-flow mode of FullModel.interpolate (U-Nets at 1/flow_scale of the size; an approximation of the
        reference's output, not parity); the canvas is then padded to multiples of 32 * flow_scale.  tile = (th, tw): the tiled mode of
        FullModel.interpolate (windows of tile + halo stitched with a cross-fade of `blend`; an approximation of the untiled output,
        not parity)."""
        from .coarse import check_scale
        from .tiles import check_args
        self.flow_scale = check_scale(flow_scale)
        if self.flow_scale != 1 and getattr(model, "recurrent", False):
            raise NotImplementedError("flow_scale=%d is not available with a recurrent bottleneck" % self.flow_scale)
        self.tile, self.halo, self.blend = (None, halo, blend) if tile is None else check_args(tile, halo, blend)
        if self.tile is not None and self.flow_scale != 1:
            raise NotImplementedError("tile=%dx%d together with flow_scale=%d: tiles are not available in the coarse-flow mode"
                                      % (self.tile + (self.flow_scale,)))
        if self.tile is not None and getattr(model, "recurrent", False):
            raise NotImplementedError("tile=%dx%d is not available with a recurrent bottleneck" % self.tile)
        n_frames = cfg.getint("TRAIN", "N_FRAMES")
        if n_frames != 2:
            raise NotImplementedError("N_FRAMES=%d needs the recurrent bottleneck (unpinned upstream); use N_FRAMES=2" % n_frames)
        if int(upsample_rate) < 2:
            raise ValueError("upsample_rate must be at least 2")
        self.model, self.cfg, self.rate = model, cfg, int(upsample_rate)
        self.n_streams, self.pb = max(1, int(n_streams)), max(1, int(pairs_per_batch))
        self.matrix, self.color_range = matrix, color_range
        self._pipe = None

    def canvas(self, h, w):
        """(Hp, Wp) of the planes an h x w clip runs on: padded_dims to multiples of 32 * flow_scale."""
        return padded_dims(h, w, 32 * self.flow_scale)[0]

    def _pipeline(self, hp, wp, dev):
        import os
        from .engine import PairPipeline
        m = self.model
        mode = m.precision or os.environ.get("SSM_PRECISION", sys.modules[type(m).__module__].DEFAULT_PRECISION)      # as FullModel.interpolate
        key = (hp, wp, str(dev), mode, self.n_streams, self.pb, self.rate, self.flow_scale, self.tile, self.halo, self.blend, m._stamp())
        if self._pipe is None or self._pipe[0] != key:
            sd1 = {k: v.detach() for k, v in m.stage1_model.state_dict().items()}
            sd2 = {k: v.detach() for k, v in m.stage2_model.state_dict().items()}
            self._pipe = None
            self._pipe = (key, PairPipeline(sd1, sd2, self.rate - 1, hp, wp, dev, m.cross_skip, mode, self.n_streams,
                                            pairs_per_batch=self.pb, flow_scale=self.flow_scale, tile=self.tile, halo=self.halo,
                                            blend=self.blend))
        return self._pipe[1]

    @torch.no_grad()
    def run(self, reader, writer):
        """Returns the number of frames written: (n - 1) * upsample_rate + 1 for n input frames."""
        from .evaluation import t_values
        h, w, siting, fb = reader.height, reader.width, reader.siting, reader.frame_bytes
        if (writer.height, writer.width, writer.siting) != (h, w, siting):
            raise ValueError("reader and writer disagree on the frame format")
        matrix = default_matrix(h) if self.matrix is None else self.matrix
        crange = self.color_range if self.color_range is not None else (reader.color_range if reader.color_range is not None else LIMITED)
        dev = next(self.model.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("the model must be on the GPU (the HIP path has no CPU fallback)")
        mult = 32 * self.flow_scale
        hp, wp = self.canvas(h, w)
        pipe = self._pipeline(hp, wp, dev)
        n, pb, nt = pipe.n, self.pb, self.rate - 1
        depth = n + 2                                                  # ring slots: one per pass in flight, one being read, one being written
        t_dev = torch.tensor(t_values(self.rate), dtype=torch.float32, device=dev)
        host_in = [torch.empty(pb, fb, dtype=torch.uint8).pin_memory() for _ in range(depth)]
        host_out = [torch.empty(pb * nt, fb, dtype=torch.uint8).pin_memory() for _ in range(depth)]
        np_in, np_out = [t.numpy() for t in host_in], [t.numpy() for t in host_out]
        done = [torch.cuda.Event() for _ in range(depth)]
        dev_in = [torch.empty(pb, fb, dtype=torch.uint8, device=dev) for _ in range(n)]
        dev_out = [torch.empty(pb * nt, fb, dtype=torch.uint8, device=dev) for _ in range(n)]
        planes = [torch.empty(pb + 1, 3, hp, wp, dtype=torch.float32, device=dev) for _ in range(n)]      # [carried left frame | new frames]
        ingested = [torch.cuda.Event() for _ in range(n)]
        first = torch.empty(1, fb, dtype=torch.uint8).pin_memory()
        if not reader.read_frame_into(first.numpy()[0]):
            raise Y4MError("the Y4M stream holds no frame")
        torch.cuda.synchronize(dev)

        free, work, failure = queue.Queue(), queue.Queue(), []
        for r in range(depth):
            free.put(r)

        def drain():
            while True:
                item = work.get()
                if item is None:
                    return
                r, valid = item
                try:
                    if not failure:
                        if r < 0:
                            writer.write_frame(first.numpy()[0])
                        else:
                            done[r].synchronize()
                            for kind, row in pass_order(valid, nt):
                                writer.write_frame(np_out[r][row] if kind == "interp" else np_in[r][row])
                except BaseException as e:          # noqa: BLE001 - handed to the caller's thread; keep releasing slots
                    failure.append(e)
                if r >= 0:
                    free.put(r)

        th = threading.Thread(target=drain, name="y4m-writer", daemon=True)
        th.start()
        written = 1
        try:
            work.put((-1, 0))
            # frame 0: ingested where pass 0 looks for its carried left frame
            last = (n - 1) % n
            with torch.cuda.stream(pipe.streams[last]):
                dev_in[last][:1].copy_(first, non_blocking=True)
                frames_from_yuv(dev_in[last][:1], h, w, siting, matrix, crange, self.cfg, True, out=planes[last][pb:], multiple=mult)
                ingested[last].record()
            j, eof = 0, False
            while not eof and not failure:
                r = free.get()
                valid = 0
                while valid < pb and reader.read_frame_into(np_in[r][valid]):
                    valid += 1
                if valid < pb:
                    eof = True
                    if valid == 0:
                        free.put(r)
                        break
                    np_in[r][valid:] = np_in[r][valid - 1]          # fill the pass; the extra pairs are not written
                k, kprev = j % n, (j - 1) % n
                st = pipe.streams[k]
                with torch.cuda.stream(st):
                    dev_in[k].copy_(host_in[r], non_blocking=True)
                    st.wait_event(ingested[kprev])
                    planes[k][0].copy_(planes[kprev][pb])
                    frames_from_yuv(dev_in[k], h, w, siting, matrix, crange, self.cfg, True, out=planes[k][1:], multiple=mult)
                    ingested[k].record()
                    x = planes[k]
                    img6 = x.view(1, 6, hp, wp) if pb == 1 else x.as_strided((pb, 6, hp, wp), (3 * hp * wp, hp * wp, wp, 1))
                    frames = pipe.engines[k].run(img6, t_dev, False)
                    frames_to_yuv(frames, h, w, siting, matrix, crange, self.cfg, out=dev_out[k])
                    host_out[r].copy_(dev_out[k], non_blocking=True)
                    done[r].record()
                work.put((r, valid))
                written += valid * self.rate
                j += 1
        finally:
            work.put(None)
            th.join()
            torch.cuda.synchronize(dev)
        if failure:
            raise failure[0]
        return written
