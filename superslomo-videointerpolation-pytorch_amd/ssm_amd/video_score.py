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

With the repository's synthetic weights the numbers say nothing about quality: they show that the instrument works.

Out of scope: a frame-blend baseline, SSIM and VMAF, scoring the timeline and shutter modes (target_rate, speed, shutter) or scene cuts -
none has a held-out counterpart on the fixed grid -, the recurrent configuration.
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


def plane_sse_host(payload_a, payload_b, h, w, siting, bits=8):
    """Yardstick of ssm_plane_sse_fwd: [N, frame_bytes] uint8 payloads (numpy; either may have one row, compared against all of the
    other's) -> uint64 [N,3], out[n][p] = the sum over plane p (Y, U, V) of (a - b)^2, exact.  8-bit planes are summed in int64.  Samples of
    more than 8 bits are 16-bit words of which ALL 16 bits count, as in the kernel: a row of a plane is summed in int64 (a difference
    squared is below 2^32, a row of fewer than 2^31 samples cannot overflow), the rows as Python integers.  The result is exact while a
    sum is below 2^64, which only a plane of more than 2^32 samples can reach: beyond any real frame."""
    fb = V.frame_bytes(h, w, siting, bits)
    a = np.ascontiguousarray(payload_a).reshape(-1, fb)
    b = np.ascontiguousarray(payload_b).reshape(-1, fb)
    assert a.dtype == np.uint8 and b.dtype == np.uint8
    n = max(a.shape[0], b.shape[0])
    assert a.shape[0] in (1, n) and b.shape[0] in (1, n), "as many payloads in a as in b, or one"
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
    fb = V.frame_bytes(h, w, siting, bits)
    for t in (payload_a, payload_b):
        assert t.is_cuda and t.dtype == torch.uint8 and t.dim() == 2 and t.shape[1] >= fb and (t.shape[1] == 1 or t.stride(1) == 1), \
            "payloads must be [N, at least frame_bytes] uint8 tensors on the GPU with unit stride within a frame"
    n = payload_a.shape[0]
    assert payload_b.shape[0] == n and payload_b.device == payload_a.device, "as many frames in a as in b, on one device"
    if out is None:
        out = torch.empty(n, 3, dtype=torch.int64, device=payload_a.device)
    assert out.is_cuda and out.dtype == torch.int64 and tuple(out.shape) == (n, 3) and out.is_contiguous()
    sa, sb = (t.stride(0) if n > 1 else 0 for t in (payload_a, payload_b))          # the stride of a single row names nothing
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
    """What HoldOutScorer.run() returns.  frames: [(i, k, sse_model (y, u, v), sse_nearest (y, u, v))] of every scored frame, Python ints,
    in clip order; frames_read, kept, trailing (frames after the last kept one: read, not scored), written (frames handed to the writer,
    or dropped without one); samples: (Y, U, V) of a frame; hold, bits."""

    PLANES = ("y", "u", "v", "avg")

    def __init__(self, hold, bits, samples):
        self.hold, self.bits, self.samples = hold, bits, tuple(samples)
        self.frames, self.frames_read, self.kept, self.trailing, self.written = [], 0, 0, 0, 0

    @property
    def scored(self):
        return len(self.frames)

    def pooled(self, k=None):
        """{"frames": count, "model": {y, u, v, avg}, "nearest": {...}} at position k (None: every position): PSNR of the pooled MSE,
        sum of sse over the frames / sum of samples; None when no frame is scored there."""
        rows = [f for f in self.frames if k is None or f[1] == k]
        if not rows:
            return None
        out = {"frames": len(rows)}
        for name, col in (("model", 2), ("nearest", 3)):
            sse = [sum(f[col][p] for f in rows) for p in range(3)]
            smp = [s * len(rows) for s in self.samples]
            out[name] = dict(zip(self.PLANES, [psnr(sse[p], smp[p], self.bits) for p in range(3)] + [psnr_avg(sse, smp, self.bits)]))
        return out

    def worst(self):
        """(PSNR-Y of `model`, frame index) of the frame where it is least; None when nothing is scored."""
        if not self.frames:
            return None
        return min((psnr(f[2][0], self.samples[0], self.bits), f[0]) for f in self.frames)

    def stats_lines(self):
        """One line per scored frame, in the manner of ffmpeg's psnr stats file."""
        lines = []
        for i, k, m, nr in self.frames:
            lines.append("n:%d k:%d mse_y %.6f psnr_y %.4f psnr_u %.4f psnr_v %.4f psnr_avg %.4f nearest_psnr_y %.4f" % (
                i, k, m[0] / self.samples[0], psnr(m[0], self.samples[0], self.bits), psnr(m[1], self.samples[1], self.bits),
                psnr(m[2], self.samples[2], self.bits), psnr_avg(m, self.samples, self.bits), psnr(nr[0], self.samples[0], self.bits)))
        return lines

    def table(self):
        """The summary as text: a row per position k and one for all, model beside nearest; the worst frame; what was not scored."""
        head = "%-6s %6s | %8s %8s %8s %8s | %8s %8s %8s %8s" % (("k", "frames") + tuple("model_" + p for p in self.PLANES)[:4]
                                                                   + tuple("near_" + p for p in self.PLANES))
        lines = ["hold-out score, hold = %d: %d frames read, %d kept, %d scored, %d trailing and not scored (PSNR in dB of the pooled MSE, "
                 "peak %d)" % (self.hold, self.frames_read, self.kept, self.scored, self.trailing, (1 << self.bits) - 1)]
        if not self.frames:
            return "\n".join(lines + ["nothing scored: a held-out frame needs a kept frame on either side, a clip of more than hold = %d "
                                      "frames" % self.hold])
        lines.append(head)
        for k in list(range(1, self.hold)) + [None]:
            r = self.pooled(k)
            if r is None:
                continue
            lines.append("%-6s %6d | %s | %s" % ("all" if k is None else "%d/%d" % (k, self.hold), r["frames"],
                                                " ".join("%8.3f" % r["model"][p] for p in self.PLANES),
                                                " ".join("%8.3f" % r["nearest"][p] for p in self.PLANES)))
        db, i = self.worst()
        lines.append("worst frame: PSNR-Y %.3f dB at input frame %d" % (db, i))
        return "\n".join(lines)


# ---- the streamed loop ------------------------------------------------------------------------------------------------------------------
class HoldOutScorer:
    """reader -> the clip scored against its own held-out frames (module docstring), streamed; with a writer, the clip that
    VideoInterpolator(upsample_rate=hold) writes for the decimated input comes out as well, byte for byte.

    The options are VideoInterpolator's where they have a held-out counterpart; target_rate, speed, shutter and scene_cut have none and
    are not offered.  The pair pipeline is the one VideoInterpolator(upsample_rate=hold, ...) builds: it is built by one.

    A pass takes pairs_per_batch groups of the clip: the group's hold - 1 held-out payloads and the kept frame that closes it.  For the
    kept frames it is VideoInterpolator._run_fixed's pass call for call - H2D, ingest of the kept payloads only, the engine, egress, D2H.
    On top: the H2D of the held-out payloads, which never go through ingest; the `nearest` calls - one ssm_plane_sse_fwd per kept frame
    of the pass, its payload (stride 0) against the run of held-out payloads it is the nearer one of; and, after egress, one `model`
    call over the pass's synthesised payloads against its held-out ones.  The sums go back to the pass's pinned ring slot ahead of `done`,
    as the scene cuts' do, and the writer thread turns them into the result's rows.  Nothing synchronises the host inside the loop but
    the ring.  Host and device memory are fixed by the frame size, hold, n_streams and pairs_per_batch.

    The left kept payload of a pass's first pair is carried on the device the way the scene cuts carry their luma row: row 0 in front of a
    stream's kept payloads, written by the pass before into the NEXT stream's buffer.  That is why the `nearest` calls sit ahead of
    `ingested` and not behind the egress: the pass that writes row 0 does so after its own calls and before it records `ingested`, the
    pass that reads it waits for that event, and the pass that read the row before recorded its own event - after its calls - earlier in
    the chain of waits.  They need nothing that the engine makes."""

    def __init__(self, model, cfg, hold, n_streams=2, pairs_per_batch=1, matrix=None, color_range=None, flow_scale=1, tile=None, halo=256,
                 blend=32):
        hold_out_plan(0, hold)          # refuses a bad hold by name
        self.hold = int(hold)
        self.vi = V.VideoInterpolator(model, cfg, upsample_rate=self.hold, n_streams=n_streams, pairs_per_batch=pairs_per_batch,
                                      matrix=matrix, color_range=color_range, flow_scale=flow_scale, tile=tile, halo=halo, blend=blend)

    @torch.no_grad()
    def run(self, reader, writer=None, on_frame=None):
        """Scores the clip and returns a HoldOutResult.  writer: a Y4MWriter of the reader's format, or None to drop the frames;
        on_frame(i, k, sse_model, sse_nearest): called on the writer thread for every scored frame as its pass completes, in clip order."""
        from .evaluation import t_values
        vi, hold = self.vi, self.hold
        clip = vi._clip(reader, reader if writer is None else writer)
        h, w, siting, bits = reader.height, reader.width, reader.siting, getattr(reader, "bits", 8)
        res = HoldOutResult(hold, bits, plane_samples(h, w, siting))
        fb, dev, hp, wp = clip.fb, clip.dev, clip.hp, clip.wp
        pipe = vi._pipeline(hp, wp, dev)
        n, pb, nt, nl = pipe.n, vi.pb, hold - 1, nearest_split(hold)
        depth = n + 2
        t_dev = torch.tensor(t_values(hold), dtype=torch.float32, device=dev)
        host_in, host_out, _, np_in, np_out, _, done = V.ring_slots(depth, fb, pb, pb * nt)
        host_held = [torch.empty(pb * nt, fb, dtype=torch.uint8).pin_memory() for _ in range(depth)]
        np_held = [t.numpy() for t in host_held]
        host_sums = [torch.empty(2, pb * nt, 3, dtype=torch.int64).pin_memory() for _ in range(depth)]          # [model | nearest]
        np_sums = [t.numpy().view(np.uint64) for t in host_sums]
        dev_in, dev_out, _, ingested = V.stream_buffers(n, dev, fb, 1 + pb, pb * nt)          # row 0: the carried left kept payload
        dev_held = [torch.empty(pb * nt, fb, dtype=torch.uint8, device=dev) for _ in range(n)]
        dev_sums = [torch.zeros(2, pb * nt, 3, dtype=torch.int64, device=dev) for _ in range(n)]
        planes = [torch.empty(pb + 1, 3, hp, wp, dtype=torch.float32, device=dev) for _ in range(n)]
        first = torch.empty(1, fb, dtype=torch.uint8).pin_memory()
        if not reader.read_frame_into(first.numpy()[0]):
            raise V.Y4MError("the Y4M stream holds no frame")
        res.frames_read = res.kept = 1
        torch.cuda.synchronize(dev)

        def rows_of(r, valid, g0):
            """On the writer thread, once the pass has come: the result's rows of its `valid` groups from group g0 on, then the frames."""
            for p in range(valid):
                for k in range(1, hold):
                    o = p * nt + k - 1
                    row = ((g0 + p) * hold + k, k, tuple(int(x) for x in np_sums[r][0, o]), tuple(int(x) for x in np_sums[r][1, o]))
                    res.frames.append(row)
                    if on_frame is not None:
                        on_frame(*row)
            for kind, row in V.pass_order(valid, nt):
                yield np_out[r][row] if kind == "interp" else np_in[r][row]

        res.written = 1
        with V.PassRing(depth, writer, lambda: torch.cuda.synchronize(dev)) as ring:
            ring.hand(None, None, [first.numpy()[0]])
            last = (n - 1) % n
            with torch.cuda.stream(pipe.streams[last]):
                new = dev_in[last][1:]
                new[:1].copy_(first, non_blocking=True)
                clip.ingest(new[:1], planes[last][pb:])
                dev_in[0][0].copy_(new[0])
                ingested[last].record()
            j, eof = 0, False
            while not eof and not ring.failure:
                r = ring.take()
                valid = pending = 0          # whole groups read into the slot; held-out frames of a group that is not whole yet
                while valid < pb:
                    into = np_held[r][valid * nt + pending] if pending < nt else np_in[r][valid]
                    if not reader.read_frame_into(into):
                        break
                    res.frames_read += 1
                    pending += 1
                    if pending == hold:
                        valid, pending = valid + 1, 0
                if valid < pb:
                    eof = True
                    res.trailing = pending
                    if valid == 0:
                        ring.hand(r, None, [])
                        break
                    np_in[r][valid:] = np_in[r][valid - 1]          # fill the pass; the extra pairs are neither scored nor written
                res.kept += valid
                k, kprev, m = j % n, (j - 1) % n, valid * nt
                st = pipe.streams[k]
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
                            plane_sse(dev_held[k][lo:hi], dev_in[k][q:q + 1].expand(hi - lo, fb), h, w, siting, bits, out=dev_sums[k][1, lo:hi])
                    dev_in[(j + 1) % n][0].copy_(dev_in[k][pb])
                    ingested[k].record()
                    x = planes[k]
                    img6 = x.view(1, 6, hp, wp) if pb == 1 else x.as_strided((pb, 6, hp, wp), (3 * hp * wp, hp * wp, wp, 1))
                    frames = pipe.engines[k].run(img6, t_dev, False)
                    clip.egress(frames, dev_out[k])
                    host_out[r].copy_(dev_out[k], non_blocking=True)
                    plane_sse(dev_out[k][:m], dev_held[k][:m], h, w, siting, bits, out=dev_sums[k][0, :m])
                    host_sums[r].copy_(dev_sums[k], non_blocking=True)
                    done[r].record()
                ring.hand(r, done[r], functools.partial(rows_of, r, valid, (res.kept - 1) - valid))
                res.written += valid * hold
                j += 1
        return res

