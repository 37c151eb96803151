"""Hold-out scoring of the streamed video path: a clip scored against its own held-out frames, on the GPU.

Of a high-rate clip every `hold`-th frame is kept, the frames in between are synthesised by the pipeline that
VideoInterpolator(upsample_rate=hold) runs, and what comes out is compared with the real frames that were left out - the procedure of the
reference's evaluate_interpolation_results.py on Adobe240, and what `ffmpeg -lavfi psnr` reports for two clips - on the streamed loop:
at the tool's own rate, in every mode (flow_scale, tile) and every pixel format the tool reads, in memory that does not depend on the
clip's length.

  plane_sse_host / plane_sse   per frame pair and plane (Y, U, V) the exact sum of squared differences of the samples as they stand in the
                               payloads, by numpy (the yardstick) and by ssm_plane_sse_fwd (csrc/ssm_video.hip) on the device
  psnr / psnr_avg              10 log10(peak^2 samples / sse) in float64, peak = 2^bits - 1 whatever the code range (ffmpeg's convention);
                               planes pooled by their sums, never by their dB
  hold_out_plan                which frames of an n-frame clip are kept, held out, and read without a score (no GPU in it)
  HoldOutScorer / HoldOutResult   the streamed loop and what it reports: per held-out frame the sums of `model` (the egressed synthesised
                               payload against the held-out one: the codes the tool would write, after quantisation) and of `nearest` (the
                               held-out payload against the nearer kept frame's: the do-nothing baseline a model has to beat), per position
                               k and overall the PSNR of the pooled MSE, the worst frame
  plane_ssim_host / plane_ssim   per frame pair and plane the SSIM of x264 and of ffmpeg's `ssim` filter (4 x 4 blocks, 8 x 8 windows at
                               stride 4) as an exact integer: every window's quotient, one float64 division, is rounded to a multiple of
                               2^-32 and the windows are summed in int64 - by numpy (the yardstick; include/ssm_hip.h has the definition)
                               and by ssm_plane_ssim_fwd.  ssim_constants, plane_windows, ssim_value, ssim_db go with it.  Planes, frames
                               and positions pool by sums and window counts: "avg" is pooled by WINDOWS, not ffmpeg's plane-size weighting
  payload_mix_host / payload_mix   the cross-fade (a (den - k) + b k + den // 2) // den of two payloads, by numpy and by ssm_payload_mix_fwd
  HoldOutScorer(ssim=True, mix=True)   `mix`: a third column, the held-out payload against the cross-fade of its two kept frames at
                               k / hold - what frame blending, and every cheap rate converter, writes; on slow motion it beats `nearest`
                               by several dB, so it is the baseline an interpolator has to beat.  `ssim`: the SSIM sums of every column
                               that is on, beside its squared differences

With the repository's synthetic weights the numbers say nothing about quality: they show that the instrument works.

Out of scope: VMAF, ffmpeg's plane-size weighting for the SSIM of "All", scoring the timeline and shutter modes (target_rate, speed,
shutter) or scene cuts - none has a held-out counterpart on the fixed grid -, the recurrent configuration.  Open: the fixed cost of the
clear-plus-kernel pair that every sum call queues.
"""
import functools
import math

import numpy as np
import torch

from . import hipbind as hb
from . import video as V


# ---- the comparison -------------------------------------------------------------------------------------------------------------------
def plane_samples(h, w, siting):
    """(samples of Y, of U, of V) of one frame."""
    ch, cw = V.chroma_dims(h, w, siting)
    return h * w, ch * cw, ch * cw


def _host_pair(payload_a, payload_b, h, w, siting, bits):
    """The operands of a host yardstick: each as uint8 [its payloads, frame_bytes], and n, the pairs they make - as many payloads in a
    as in b, or one that is compared against all of the other's."""
    fb = V.frame_bytes(h, w, siting, bits)
    a = np.ascontiguousarray(payload_a).reshape(-1, fb)
    b = np.ascontiguousarray(payload_b).reshape(-1, fb)
    assert a.dtype == np.uint8 and b.dtype == np.uint8
    n = max(a.shape[0], b.shape[0])
    assert a.shape[0] in (1, n) and b.shape[0] in (1, n), "as many payloads in a as in b, or one"
    return a, b, n


def _pair_operands(payload_a, payload_b, h, w, siting, bits, out):
    """video._pair_operands for whole payloads and sums per plane: (N, out [N,3], stride of a, of b)."""
    return V._pair_operands(payload_a, payload_b, V.frame_bytes(h, w, siting, bits), "frame_bytes", out, (3,))


def plane_sse_host(payload_a, payload_b, h, w, siting, bits=8):
    """Yardstick of ssm_plane_sse_fwd: [N, frame_bytes] uint8 payloads (numpy; either may have one row, compared against all of the
    other's) -> uint64 [N,3], out[n][p] = the sum over plane p (Y, U, V) of (a - b)^2, exact.  8-bit planes are summed in int64.  Samples of
    more than 8 bits are 16-bit words of which ALL 16 bits count, as in the kernel: a row of a plane is summed in int64 (a difference
    squared is below 2^32, a row of fewer than 2^31 samples cannot overflow), the rows as Python integers.  The result is exact while a
    sum is below 2^64, which only a plane of more than 2^32 samples can reach: beyond any real frame."""
    a, b, n = _host_pair(payload_a, payload_b, h, w, siting, bits)
    out = np.zeros((n, 3), dtype=np.uint64)
    for p, (pa, pb) in enumerate(zip(V.split_planes(a, h, w, siting, bits), V.split_planes(b, h, w, siting, bits))):
        d = pa.astype(np.int64) - pb.astype(np.int64)          # [n | 1, rows, cols], broadcast over n
        d = np.broadcast_to(d * d, (n,) + d.shape[1:])
        if bits == 8:
            out[:, p] = d.reshape(n, -1).sum(axis=1).astype(np.uint64)
        else:
            rows = d.sum(axis=2)
            for i in range(n):
                out[i, p] = sum(int(r) for r in rows[i])
    return out


def plane_sse(payload_a, payload_b, h, w, siting, bits=8, out=None):
    """ssm_plane_sse_fwd on payloads: [N, at least frame_bytes] uint8 device tensors with unit stride within a row and any row stride -
    views of one buffer, frames n and n + 1, a negative step through as_strided, or a 0-stride expand of one row: one payload against N -
    -> int64 [N,3] on the device (into `out` if given), out[n][p] = the sum over plane p (Y, U, V) of (a_n - b_n)^2.  The words are
    unsigned: read them on the host as numpy uint64.  bits > 8: the bytes are 16-bit little-endian samples, all 16 bits count."""
    n, out, sa, sb = _pair_operands(payload_a, payload_b, h, w, siting, bits, out)
    hb.check(hb.load().ssm_plane_sse_fwd(payload_a.data_ptr(), payload_b.data_ptr(), sa, sb, n, h, w, siting, V.sample_bytes(bits),
                                         out.data_ptr(), hb.stream_ptr()))
    return out


def psnr(sse, samples, bits):
    """10 log10(peak^2 samples / sse) in float64 with peak = 2^bits - 1 - the full scale of the sample whatever the code range, so a
    limited-range clip is scored against 255, not 219: the convention of ffmpeg's `psnr` filter, whose numbers these are meant to sit
    beside.  inf at sse = 0."""
    sse, samples = int(sse), int(samples)
    assert sse >= 0 and samples > 0
    if sse == 0:
        return math.inf
    peak = (1 << int(bits)) - 1
    return 10.0 * math.log10(peak * peak * samples / sse)


def psnr_avg(sse3, samples3, bits):
    """The three planes pooled: PSNR of (sum of sse) / (sum of samples) - ffmpeg's `average` -, not the mean of the planes' dB."""
    return psnr(sum(int(s) for s in sse3), sum(int(s) for s in samples3), bits)


# ---- SSIM in fixed point ----------------------------------------------------------------------------------------------------------------
SSIM_ONE = 1 << 32          # fx of a window whose quotient is 1


def ssim_constants(bits):
    """(c1, c2) = (floor(.01^2 peak^2 64 + .5), floor(.03^2 peak^2 64 63 + .5)) with peak = 2^bits - 1, in exact integer arithmetic: x264's
    ssim_c1 and ssim_c2 (416 and 235963 at 8 bits).  The one function behind the yardstick and the device call."""
    V.sample_bytes(bits)
    peak2 = ((1 << int(bits)) - 1) ** 2
    return (2 * 64 * peak2 + 10000) // 20000, (2 * 9 * 64 * 63 * peak2 + 10000) // 20000


def _windows(rows, cols):
    return max(0, (rows >> 2) - 1) * max(0, (cols >> 2) - 1)


def plane_windows(h, w, siting):
    """(windows of Y, of U, of V) of one frame: max(0, (cols >> 2) - 1) max(0, (rows >> 2) - 1) of each plane."""
    ch, cw = V.chroma_dims(h, w, siting)
    return _windows(h, w), _windows(ch, cw), _windows(ch, cw)


def _block_sums(x):
    """[n, rows, cols] int64 -> [n, rows >> 2, cols >> 2]: the sums of the 4 x 4 blocks; trailing rows and columns belong to none."""
    n, rows, cols = x.shape
    by, bx = rows >> 2, cols >> 2
    return x[:, :4 * by, :4 * bx].reshape(n, by, 4, bx, 4).sum(axis=(2, 4))


def _window_sums(s):
    """Block sums -> the sums of the 2 x 2 blocks of every window, at stride one block."""
    return s[:, :-1, :-1] + s[:, :-1, 1:] + s[:, 1:, :-1] + s[:, 1:, 1:]


def plane_ssim_host(payload_a, payload_b, h, w, siting, bits=8):
    """Yardstick of ssm_plane_ssim_fwd (include/ssm_hip.h has the definition): payloads as for plane_sse_host -> int64 [N,3], out[n][p] =
    the sum over the windows of plane p of fx = rint(q 2^32), q = (double(f0) double(f1)) / (double(f2) double(f3)).  The factors are
    int64 throughout (below 2^45 at 16 bits); the three float64 operations and the scaling are numpy's, one rounding each; np.rint rounds
    half to even.  A plane without a window gives 0."""
    a, b, n = _host_pair(payload_a, payload_b, h, w, siting, bits)
    c1, c2 = (np.int64(c) for c in ssim_constants(bits))
    out = np.zeros((n, 3), dtype=np.int64)
    for p, (pa, pb) in enumerate(zip(V.split_planes(a, h, w, siting, bits), V.split_planes(b, h, w, siting, bits))):
        if _windows(pa.shape[1], pa.shape[2]) == 0:
            continue
        x, y = pa.astype(np.int64), pb.astype(np.int64)
        s1, s2 = _window_sums(_block_sums(x)), _window_sums(_block_sums(y))                 # [n | 1, wy, wx], broadcast over n below
        ss = _window_sums(_block_sums(x * x)) + _window_sums(_block_sums(y * y))
        s12 = _window_sums(_block_sums(x * y))
        var = 64 * ss - s1 * s1 - s2 * s2
        covar = 64 * s12 - s1 * s2
        f0, f1, f2, f3 = 2 * s1 * s2 + c1, 2 * covar + c2, s1 * s1 + s2 * s2 + c1, var + c2
        q = (f0.astype(np.float64) * f1.astype(np.float64)) / (f2.astype(np.float64) * f3.astype(np.float64))
        fx = np.rint(q * np.float64(SSIM_ONE)).astype(np.int64)
        out[:, p] = np.broadcast_to(fx, (n,) + fx.shape[1:]).reshape(n, -1).sum(axis=1)
    return out


def plane_ssim(payload_a, payload_b, h, w, siting, bits=8, out=None):
    """ssm_plane_ssim_fwd on payloads, shaped like plane_sse -> int64 [N,3] on the device (into `out` if given): signed sums of fx."""
    n, out, sa, sb = _pair_operands(payload_a, payload_b, h, w, siting, bits, out)
    c1, c2 = ssim_constants(bits)
    hb.check(hb.load().ssm_plane_ssim_fwd(payload_a.data_ptr(), payload_b.data_ptr(), sa, sb, n, h, w, siting, V.sample_bytes(bits), c1, c2,
                                          out.data_ptr(), hb.stream_ptr()))
    return out


def ssim_value(total, count):
    """The SSIM of `count` windows whose fx sum to `total`: total / (2^32 count) in float64; nan where there is no window."""
    total, count = int(total), int(count)
    assert count >= 0
    return math.nan if count == 0 else total / (SSIM_ONE * count)          # Python's int / int: the correctly rounded quotient


def ssim_db(ssim):
    """-10 log10(1 - ssim), ffmpeg's dB of an SSIM; inf at 1."""
    return math.inf if ssim >= 1.0 else -10.0 * math.log10(1.0 - ssim)


# ---- the cross-fade ---------------------------------------------------------------------------------------------------------------------
def mix_divisor(den):
    """(m, shift) of the kernel's division by den (Granlund and Montgomery): with l = ceil(log2 den), m = floor(2^32 (2^l - den) / den) + 1
    and shift = l - 1;  x // den = (t + ((x - t) >> 1)) >> shift  with t = (m x) >> 32, for every x below 2^32."""
    den = int(den)
    assert 2 <= den <= 65535
    l = (den - 1).bit_length()
    return (((1 << l) - den) << 32) // den + 1, l - 1


def mix_divide(x, den):
    """The kernel's quotient of numpy uint64 numerators below 2^32 by den: mix_divisor's pair applied as the kernel applies it."""
    m, shift = mix_divisor(den)
    x = np.asarray(x, dtype=np.uint64)
    t = (np.uint64(m) * x) >> np.uint64(32)
    return (t + ((x - t) >> np.uint64(1))) >> np.uint64(shift)


def payload_mix_host(payload_a, payload_b, n, num0, num_step, den, bits=8):
    """Yardstick of ssm_payload_mix_fwd: [n | 1, row bytes] uint8 payloads -> [n, row bytes] uint8, row i = (a (den - k) + b k + den // 2)
    // den with k = num0 + i num_step over the samples (bytes, or little-endian words above 8 bits), in int64 with numpy's floor division."""
    a, b = np.ascontiguousarray(payload_a), np.ascontiguousarray(payload_b)
    assert a.dtype == np.uint8 and b.dtype == np.uint8 and a.ndim == 2 and b.ndim == 2 and a.shape[1] == b.shape[1]
    assert a.shape[0] in (1, n) and b.shape[0] in (1, n) and 2 <= den <= 65535
    dt = np.uint8 if V.sample_bytes(bits) == 1 else "<u2"
    k = (num0 + num_step * np.arange(n, dtype=np.int64))[:, None]
    assert k.min() >= 0 and k.max() <= den
    x, y = a.view(dt).astype(np.int64), b.view(dt).astype(np.int64)
    return np.ascontiguousarray(((x * (den - k) + y * k + den // 2) // den).astype(dt)).view(np.uint8).reshape(n, -1)


def payload_mix(payload_a, payload_b, num0, num_step, den, bits=8, out=None, samples=None):
    """ssm_payload_mix_fwd: [N, L] uint8 device tensors with unit stride within a row and any row stride (0: one payload for every row) ->
    `out` [N, at least L] (made if None); `samples`: how many samples of a row are mixed (default: all L bytes of it)."""
    sb = V.sample_bytes(bits)
    n, length = payload_a.shape
    for t in (payload_a, payload_b):
        assert t.is_cuda and t.dtype == torch.uint8 and t.dim() == 2 and tuple(t.shape) == (n, length) and (length == 1 or t.stride(1) == 1)
    if samples is None:
        assert length % sb == 0
        samples = length // sb
    assert 0 < samples * sb <= length
    if out is None:
        out = torch.empty(n, length, dtype=torch.uint8, device=payload_a.device)
    assert out.is_cuda and out.dtype == torch.uint8 and out.dim() == 2 and out.shape[0] == n and out.shape[1] >= samples * sb
    assert out.shape[1] == 1 or out.stride(1) == 1
    sa, sb_, so = (t.stride(0) if n > 1 else 0 for t in (payload_a, payload_b, out))
    hb.check(hb.load().ssm_payload_mix_fwd(payload_a.data_ptr(), payload_b.data_ptr(), sa, sb_, out.data_ptr(), so, n, samples, sb, num0, num_step,
                                           den, hb.stream_ptr()))
    return out


# ---- which frames -----------------------------------------------------------------------------------------------------------------------
def hold_out_plan(n, hold):
    """(kept, held, trailing) of an n-frame clip: the kept frames 0, hold, 2 hold, ... below n; the held-out frames, every one strictly
    between two kept frames, as (i, k) with i = g hold + k; the (n - 1) mod hold frames after the last kept one, read and not scored."""
    if isinstance(hold, bool) or int(hold) != hold or hold < 2:
        raise ValueError("hold must be a whole number, at least 2 (got %r)" % (hold,))
    groups = (n - 1) // hold if n > 0 else 0
    kept = [g * hold for g in range(groups + 1)] if n > 0 else []
    held = [(g * hold + k, k) for g in range(groups) for k in range(1, hold)]
    trailing = list(range(groups * hold + 1, n))
    return kept, held, trailing


def nearest_split(hold):
    """How many of a group's hold - 1 held-out frames are nearer to the left kept frame: those with k / hold < 1/2."""
    return (hold - 1) // 2


class HoldOutResult:
    """What HoldOutScorer.run() returns.  records: one (i, k, sums) per scored frame, in clip order, sums[metric][column] = (y, u, v) as
    Python ints - metric "sse" and, with ssim on, "ssim" (the signed fixed-point sums of plane_ssim_host over `windows`, the (Y, U, V)
    window counts of a frame); column "model", "nearest" and, with mix on, "mix".  frames_read, kept, trailing (frames after the last
    kept one: read, not scored), written (frames handed to the writer, or dropped without one); samples: (Y, U, V) of a frame; hold, bits.

    Two views of the records, readable and assignable (frames first): frames = [(i, k, sse_model (y, u, v), sse_nearest (y, u, v))],
    and more, a list parallel to it with what those four fields leave out: more[j] = {"sse": {"mix": (y, u, v)}, "ssim": {"model":
    (y, u, v), "nearest": ..., "mix": ...}}, only the metrics and columns that are on, and [] when neither ssim nor mix is."""

    PLANES = ("y", "u", "v", "avg")
    SHORT = {"model": "model_", "nearest": "near_", "mix": "mix_"}          # the table's column heads
    # a stats line: per metric its name, its format, and the planes it shows of each column
    STATS = {"sse": ("psnr", "%.4f", {"model": PLANES, "nearest": ("y",), "mix": ("y", "avg")}),
             "ssim": ("ssim", "%.6f", {"model": PLANES, "nearest": ("y",), "mix": ("y",)})}

    def __init__(self, hold, bits, samples, windows=(0, 0, 0), ssim=False, mix=False):
        self.hold, self.bits, self.samples = hold, bits, tuple(samples)
        self.windows, self.ssim, self.mix = tuple(windows), bool(ssim), bool(mix)
        self.records, self.frames_read, self.kept, self.trailing, self.written = [], 0, 0, 0, 0

    @property
    def columns(self):
        """The columns that are on, in report order."""
        return ("model", "nearest") + (("mix",) if self.mix else ())

    @property
    def metrics(self):
        return ("sse",) + (("ssim",) if self.ssim else ())

    @staticmethod
    def _row(rec):
        return rec[0], rec[1], rec[2]["sse"]["model"], rec[2]["sse"]["nearest"]

    @staticmethod
    def _more(rec):
        rest = {m: {c: v for c, v in by.items() if m != "sse" or c not in ("model", "nearest")} for m, by in rec[2].items()}
        return {m: by for m, by in rest.items() if by}

    def add(self, i, k, sums):
        """Appends a scored frame's record; -> (its row of `frames`, its entry of `more`: {} with ssim and mix off)."""
        self.records.append((i, k, sums))
        return self._row(self.records[-1]), self._more(self.records[-1])

    @property
    def frames(self):
        return [self._row(rec) for rec in self.records]

    @frames.setter
    def frames(self, rows):
        self.records = [(i, k, {"sse": {"model": m, "nearest": nr}}) for i, k, m, nr in rows]

    @property
    def more(self):
        return [m for m in map(self._more, self.records) if m]

    @more.setter
    def more(self, entries):
        assert len(entries) == len(self.records), "one entry per row of frames"
        for (_, _, sums), entry in zip(self.records, entries):
            for metric, by in entry.items():
                sums.setdefault(metric, {}).update(by)

    @property
    def scored(self):
        return len(self.records)

    def _pool4(self, recs, metric, col):
        """{y, u, v, avg} of column `col` pooled over the records: the PSNR of the summed squared differences over the summed samples,
        or the SSIM of the summed fx over the summed windows; avg pools the three planes the same way."""
        tot = [sum(rec[2][metric][col][p] for rec in recs) for p in range(3)]
        cnt = [c * len(recs) for c in (self.samples if metric == "sse" else self.windows)]
        value = (lambda t, c: psnr(t, c, self.bits)) if metric == "sse" else ssim_value
        return dict(zip(self.PLANES, [value(tot[p], cnt[p]) for p in range(3)] + [value(sum(tot), sum(cnt))]))

    def pooled(self, k=None):
        """{"frames": count, column: {y, u, v, avg}, ...} at position k (None: every position) for every column that is on: PSNR of the
        pooled MSE, sum of sse over the frames / sum of samples; with ssim on, "ssim": {column: {y, u, v, avg}}, pooled by windows.
        None when no frame is scored there."""
        recs = [rec for rec in self.records if k is None or rec[1] == k]
        if not recs:
            return None
        out = {"frames": len(recs)}
        out.update((col, self._pool4(recs, "sse", col)) for col in self.columns)
        if self.ssim:
            out["ssim"] = {col: self._pool4(recs, "ssim", col) for col in self.columns}
        return out

    def worst(self):
        """(PSNR-Y of `model`, frame index) of the frame where it is least; None when nothing is scored."""
        if not self.records:
            return None
        return min((psnr(sums["sse"]["model"][0], self.samples[0], self.bits), i) for i, _, sums in self.records)

    def stats_lines(self):
        """One line per scored frame, in the manner of ffmpeg's psnr stats file: per metric all of `model`, then STATS' planes of the
        other columns under their names."""
        lines = []
        for rec in self.records:
            line = "n:%d k:%d mse_y %.6f" % (rec[0], rec[1], rec[2]["sse"]["model"][0] / self.samples[0])
            for metric in self.metrics:
                name, fmt, shown = self.STATS[metric]
                for col in self.columns:
                    v4 = self._pool4([rec], metric, col)
                    line += "".join((" %s%s_%s " + fmt) % ("" if col == "model" else col + "_", name, p, v4[p]) for p in shown[col])
            lines.append(line)
        return lines

    def _block(self, keys, metric, cols, width, digits):
        """Lines of the table: a head, then per position the {y, u, v, avg} of the columns `cols` side by side."""
        cell = "%%%d.%df" % (width, digits)
        lines = ["%-6s %6s | %s" % ("k", "frames", " | ".join(" ".join("%*s" % (width, self.SHORT[c] + p) for p in self.PLANES) for c in cols))]
        for name, r in keys:
            by = r if metric == "sse" else r[metric]
            lines.append("%-6s %6d | %s" % (name, r["frames"], " | ".join(" ".join(cell % by[c][p] for p in self.PLANES) for c in cols)))
        return lines

    def table(self):
        """The summary as text: a row per position k and one for all, model beside nearest; the worst frame; what was not scored; then a
        block for the PSNR of `mix` and one for the SSIM of every column, where they are on."""
        lines = ["hold-out score, hold = %d: %d frames read, %d kept, %d scored, %d trailing and not scored (PSNR in dB of the pooled MSE, "
                 "peak %d)" % (self.hold, self.frames_read, self.kept, self.scored, self.trailing, (1 << self.bits) - 1)]
        if not self.records:
            return "\n".join(lines + ["nothing scored: a held-out frame needs a kept frame on either side, a clip of more than hold = %d "
                                      "frames" % self.hold])
        keys = [(k, self.pooled(k)) for k in list(range(1, self.hold)) + [None]]
        keys = [("all" if k is None else "%d/%d" % (k, self.hold), r) for k, r in keys if r is not None]
        lines += self._block(keys, "sse", self.columns[:2], 8, 3)
        lines.append("worst frame: PSNR-Y %.3f dB at input frame %d" % self.worst())
        if self.columns[2:]:
            lines.append("mix: the held-out frame against the cross-fade of its two kept frames at k / hold (PSNR in dB of the pooled MSE)")
            lines += self._block(keys, "sse", self.columns[2:], 8, 3)
        if self.ssim:
            lines.append("SSIM (8 x 8 windows at stride 4, as x264 and ffmpeg's ssim filter; sums pooled by windows - `avg` is not ffmpeg's "
                         "plane-size weighting; %d + %d + %d windows a frame)" % self.windows)
            lines += self._block(keys, "ssim", self.columns, 10, 6)
            allr = keys[-1][1]["ssim"]
            lines.append("SSIM of all frames in dB, -10 log10(1 - ssim): " + ", ".join(
                "%s Y %.3f avg %.3f" % (c, ssim_db(allr[c]["y"]), ssim_db(allr[c]["avg"])) for c in self.columns))
        return "\n".join(lines)


# ---- the streamed loop ------------------------------------------------------------------------------------------------------------------
class HoldOutScorer:
    """reader -> the clip scored against its own held-out frames (module docstring), streamed; with a writer, the clip that
    VideoInterpolator(upsample_rate=hold) writes for the decimated input comes out as well, byte for byte.

    The options are VideoInterpolator's where they have a held-out counterpart; target_rate, speed, shutter and scene_cut have none and
    are not offered.  The pair pipeline is the one VideoInterpolator(upsample_rate=hold, ...) builds: it is built by one.

    A pass takes pairs_per_batch groups of the clip: the group's hold - 1 held-out payloads and the kept frame that closes it (group_reader,
    the unit reader of video.read_blocks: the passes, the short and the empty last one and the ring's failure protocol are the fixed
    grid's, through VideoInterpolator._run_passes).  For the kept frames what a pass queues is VideoInterpolator._run_fixed's without
    options, call for call - H2D, ingest of the kept payloads only, the engine, egress, D2H.
    On top: the H2D of the held-out payloads, which never go through ingest; the `nearest` calls - one ssm_plane_sse_fwd per kept frame
    of the pass, its payload (stride 0) against the run of held-out payloads it is the nearer one of; and, after egress, one `model`
    call over the pass's synthesised payloads against its held-out ones.  The sums go back to the pass's pinned ring slot ahead of `done`,
    as the scene cuts' do, and the writer thread turns them into the result's rows.  Nothing synchronises the host inside the loop but
    the ring.  Host and device memory are fixed by the frame size, hold, n_streams and pairs_per_batch.

    mix=True adds the column `mix`: per group one ssm_payload_mix_fwd call - N = hold - 1 rows, both kept payloads at stride 0, k = 1 ..
    hold - 1 over den = hold - into a per-stream buffer of the held-out payloads' shape, then one ssm_plane_sse_fwd call over the pass
    against the held-out payloads.  ssim=True adds one ssm_plane_ssim_fwd call beside every ssm_plane_sse_fwd call, over the same operands,
    for every column that is on.  With both off the loop queues what it queued before they existed, launch for launch.

    The left kept payload of a pass's first pair is carried on the device the way the scene cuts carry their luma row: row 0 in front of a
    stream's kept payloads, written by the pass before into the NEXT stream's buffer.  That is why the `nearest` and `mix` calls - both read row 0 - sit ahead of
    `ingested` and not behind the egress: the pass that writes row 0 does so after its own calls and before it records `ingested`, the
    pass that reads it waits for that event, and the pass that read the row before recorded its own event - after its calls - earlier in
    the chain of waits.  They need nothing that the engine makes.  The model's SSIM call sits beside the model's squared differences, after
    the egress.  (`blend` is the tiles' seam width, which is why the baseline is called `mix`.)"""

    def __init__(self, model, cfg, hold, n_streams=2, pairs_per_batch=1, matrix=None, color_range=None, flow_scale=1, tile=None, halo=256,
                 blend=32, ssim=False, mix=False):
        hold_out_plan(0, hold)          # refuses a bad hold by name
        self.hold = int(hold)
        self.ssim, self.mix = bool(ssim), bool(mix)
        self.vi = V.VideoInterpolator(model, cfg, upsample_rate=self.hold, n_streams=n_streams, pairs_per_batch=pairs_per_batch,
                                      matrix=matrix, color_range=color_range, flow_scale=flow_scale, tile=tile, halo=halo, blend=blend)

    @torch.no_grad()
    def run(self, reader, writer=None, on_frame=None, on_scores=None):
        """Scores the clip and returns a HoldOutResult.  writer: a Y4MWriter of the reader's format, or None to drop the frames;
        on_frame(i, k, sse_model, sse_nearest): called on the writer thread for every scored frame as its pass completes, in clip order;
        on_scores(i, k, more): with ssim or mix on, called right after it with the frame's entry of HoldOutResult.more."""
        from .evaluation import t_values
        vi, hold = self.vi, self.hold
        clip = vi._clip(reader, reader if writer is None else writer)
        h, w, siting, bits = reader.height, reader.width, reader.siting, getattr(reader, "bits", 8)
        ssim, mix = self.ssim, self.mix
        res = HoldOutResult(hold, bits, plane_samples(h, w, siting), plane_windows(h, w, siting), ssim, mix)
        cols = 3 if mix else 2          # rows of the sums: sse of model, nearest[, mix], then ssim of the same columns
        names = ("model", "nearest", "mix")[:cols]
        fb, dev, hp, wp = clip.fb, clip.dev, clip.hp, clip.wp
        pipe = vi._pipeline(hp, wp, dev)
        n, pb, nt, nl = pipe.n, vi.pb, hold - 1, nearest_split(hold)
        depth = n + 2
        t_dev = torch.tensor(t_values(hold), dtype=torch.float32, device=dev)
        host_in, host_out, _, np_in, np_out, _, done = V.ring_slots(depth, fb, pb, pb * nt)
        host_held = [torch.empty(pb * nt, fb, dtype=torch.uint8).pin_memory() for _ in range(depth)]
        np_held = [t.numpy() for t in host_held]
        host_sums = [torch.empty(cols * (2 if ssim else 1), pb * nt, 3, dtype=torch.int64).pin_memory() for _ in range(depth)]
        np_sums = [t.numpy().view(np.uint64) for t in host_sums]          # [model | nearest]: squared differences are unsigned
        np_signed = [t.numpy() for t in host_sums]                        # the SSIM rows are signed
        dev_in, dev_out, _, ingested, _ = V.stream_buffers(n, dev, fb, 1 + pb, pb * nt)          # row 0: the carried left kept payload
        dev_held = [torch.empty(pb * nt, fb, dtype=torch.uint8, device=dev) for _ in range(n)]
        dev_sums = [torch.zeros(cols * (2 if ssim else 1), pb * nt, 3, dtype=torch.int64, device=dev) for _ in range(n)]
        dev_mix = [torch.empty(pb * nt, fb, dtype=torch.uint8, device=dev) for _ in range(n)] if mix else None
        planes = [torch.empty(pb + 1, 3, hp, wp, dtype=torch.float32, device=dev) for _ in range(n)]
        first = torch.empty(1, fb, dtype=torch.uint8).pin_memory()
        V.first_frame(reader, first.numpy()[0])
        res.frames_read = res.kept = 1
        torch.cuda.synchronize(dev)
        read_group = group_reader(reader, res, hold, np_held, np_in)

        def scored(r, valid, g0):
            """On the writer thread, once the pass has come: the result's rows of its `valid` groups from group g0 on, then the frames."""
            for p in range(valid):
                for k in range(1, hold):
                    o = p * nt + k - 1
                    sums = {"sse": {c: tuple(int(x) for x in np_sums[r][ci, o]) for ci, c in enumerate(names)}}
                    if ssim:
                        sums["ssim"] = {c: tuple(int(x) for x in np_signed[r][cols + ci, o]) for ci, c in enumerate(names)}
                    row, more = res.add((g0 + p) * hold + k, k, sums)
                    if on_frame is not None:
                        on_frame(*row)
                    if more and on_scores is not None:
                        on_scores(row[0], row[1], more)
            for kind, row in V.pass_order(valid, nt):
                yield np_out[r][row] if kind == "interp" else np_in[r][row]

        def frame0(ring):
            ring.hand(None, None, [first.numpy()[0]])
            last = (n - 1) % n
            with torch.cuda.stream(pipe.streams[last]):
                new = dev_in[last][1:]
                new[:1].copy_(first, non_blocking=True)
                clip.ingest(new[:1], planes[last][pb:])
                dev_in[0][0].copy_(new[0])
                ingested[last].record()
            return 1

        def submit(j, r, valid):
            k, kprev, m = j % n, (j - 1) % n, valid * nt
            st = pipe.streams[k]

            def compare(column, a, b, rows):
                """Queues the squared differences of payloads a against b into rows `rows` of column `column` of the pass's sums, and
                with ssim on their SSIM into the same rows of the column's SSIM block."""
                plane_sse(a, b, h, w, siting, bits, out=dev_sums[k][column, rows])
                if ssim:
                    plane_ssim(a, b, h, w, siting, bits, out=dev_sums[k][cols + column, rows])

            with torch.cuda.stream(st):
                new = dev_in[k][1:]
                new.copy_(host_in[r], non_blocking=True)
                dev_held[k][:m].copy_(host_held[r][:m], non_blocking=True)
                st.wait_event(ingested[kprev])
                planes[k][0].copy_(planes[kprev][pb])
                clip.ingest(new, planes[k][1:])
                for q in range(valid + 1):          # kept row q of dev_in[k]: the right frame of group q - 1, the left one of group q
                    lo, hi = max(0, (q - 1) * nt + nl), min(m, q * nt + nl)
                    if hi > lo:
                        compare(1, dev_held[k][lo:hi], dev_in[k][q:q + 1].expand(hi - lo, fb), slice(lo, hi))
                if mix:
                    for q in range(valid):          # group q: kept rows q (left) and q + 1 (right) of dev_in[k], k = 1 .. hold - 1
                        payload_mix(dev_in[k][q:q + 1].expand(nt, fb), dev_in[k][q + 1:q + 2].expand(nt, fb), 1, 1, hold, bits,
                                    out=dev_mix[k][q * nt:(q + 1) * nt])
                    compare(2, dev_mix[k][:m], dev_held[k][:m], slice(m))
                dev_in[(j + 1) % n][0].copy_(dev_in[k][pb])
                ingested[k].record()
                x = planes[k]
                img6 = x.view(1, 6, hp, wp) if pb == 1 else x.as_strided((pb, 6, hp, wp), (3 * hp * wp, hp * wp, wp, 1))
                frames = pipe.engines[k].run(img6, t_dev, False)
                clip.egress(frames, dev_out[k])
                host_out[r].copy_(dev_out[k], non_blocking=True)
                compare(0, dev_out[k][:m], dev_held[k][:m], slice(m))
                host_sums[r].copy_(dev_sums[k], non_blocking=True)
                done[r].record()

        def rows_of(r, on_gpu, valid):
            res.kept += valid
            return functools.partial(scored, r, valid if on_gpu else 0, (res.kept - 1) - valid), valid * hold

        res.written = vi._run_passes(clip, writer, done, lambda ring, issue: V.read_blocks(ring, pb, np_in, read_group, issue),
                                     lambda valid: valid > 0, submit, rows_of, first=frame0)
        return res


def group_reader(reader, res, hold, np_held, np_in):
    """The unit reader HoldOutScorer hands to video.read_blocks: read_group(r, i) reads group i of the pass on ring slot r - its hold - 1
    held-out frames into rows i (hold - 1) .. of np_held[r], then the kept frame that closes it into np_in[r][i] - and says whether the
    group is whole.  It keeps res.frames_read, and res.trailing: the frames of the group that the end of the stream cut short."""
    def read_group(r, i):
        for pending in range(hold):
            into = np_held[r][i * (hold - 1) + pending] if pending < hold - 1 else np_in[r][i]
            if not reader.read_frame_into(into):
                res.trailing = pending
                return False
            res.frames_read += 1
        return True

    return read_group
