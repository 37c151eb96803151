"""Optical-flow evaluation around the stage-1 pass: what scripts/evaluate_optical_flow_results.py and
scripts/utils/dataloaders/sintel_opticalflow.py do around `FullModel`, restated from their behaviour.

  * `FullModel.estimate_flow` runs stage 1 alone (the reference runs the full model and keeps `intermediate_outputs[0]`);
  * `flow_metrics` / `flow_to_rgb` score and colour-code a flow field on the GPU where stage 1 left it (csrc/ssm_flow.hip);
  * `compute_metrics_host` and scripts/utils/flo_utils.py stay the yardsticks, and `FlowEvaluator(metrics="host")` the default;
  * `flow_consistency` scores a pair's two flows against each other on the GPU (forward-backward consistency: no ground truth needed),
    `flow_consistency_host` is its numpy yardstick, `FlowCheck` one pair's record, `parse_flow_check` the streamed option's parser.
"""
from collections import namedtuple
from fractions import Fraction

import numpy as np
import torch

from . import frames as F
from . import hipbind as hb


class PlaneChannels:
    """Two channels [c0, c0 + 2) of a hipbind.Planes (FullModel.estimate_flow(..., want_planes=True)) as a flow field for
    flow_metric_sums / flow_to_rgb: the kernels read the plan's own padded planes, no copy."""

    def __init__(self, planes, c0=0):
        assert 0 <= c0 and c0 + 2 <= planes.C, "channels %d..%d of a %d-channel tensor" % (c0, c0 + 1, planes.C)
        self.planes, self.c0 = planes, c0
        self.shape = (planes.B, 2, planes.H, planes.W)
        self.device = planes.buf.device

    def view(self):
        return self.planes.view(self.c0)


def _field(flow, h, w, top, left):
    """(ssm_view, N, device, tensor) of a flow argument after the checks both entry points share.  The fourth value is the tensor the view
    points into - the argument, or its contiguous copy when the x-stride was not 1 - which the caller keeps alive across the launch."""
    if isinstance(flow, PlaneChannels):
        view, shape, dev = flow.view(), flow.shape, flow.device
    else:
        if not (isinstance(flow, torch.Tensor) and flow.is_cuda and flow.dtype == torch.float32 and flow.dim() == 4
                and flow.shape[1] == 2):
            raise RuntimeError("flow must be a [N,2,H,W] float32 tensor on the GPU (or PlaneChannels); got %s %s on %s"
                               % (getattr(flow, "dtype", type(flow)), tuple(getattr(flow, "shape", ())), getattr(flow, "device", "?")))
        if flow.stride(3) != 1:
            flow = flow.contiguous()
        view, shape, dev = hb.view_of(flow), tuple(flow.shape), flow.device
    if not (h >= 1 and w >= 1 and top >= 0 and left >= 0 and top + h <= shape[2] and left + w <= shape[3]):
        raise RuntimeError("crop %dx%d at (%d, %d) does not fit the %dx%d flow" % (h, w, top, left, shape[2], shape[3]))
    return view, shape[0], dev, flow


def flow_metric_sums(flow, gt, top=0, left=0, mode=0):
    """Per-field sums of ssm_flow_metrics_fwd: float64 [N,3] on the device = (sum of end-point errors, pixels more than 3 px off,
    pixels counted).  flow: [N,2,*,*] float32 device tensor (any strides with unit x-stride: a channel slice of the 4-channel
    stage-1 output works) or PlaneChannels; gt: [N,H,W,2] float32 device tensor, the .flo layout; the flow is cropped at
    (top, left) to gt's H x W.  mode 0: every pixel (compute_metrics); 1: known, non-zero ground truth only (flow_error).
    Launched on the current stream; no synchronisation."""
    if not (isinstance(gt, torch.Tensor) and gt.is_cuda and gt.dtype == torch.float32 and gt.dim() == 4 and gt.shape[3] == 2):
        raise RuntimeError("ground truth must be a [N,H,W,2] float32 tensor on the GPU; got %s %s on %s"
                           % (getattr(gt, "dtype", type(gt)), tuple(getattr(gt, "shape", ())), getattr(gt, "device", "?")))
    n, h, w, _ = gt.shape
    view, nf, dev, keep = _field(flow, h, w, top, left)
    if nf != n or dev != gt.device:
        raise RuntimeError("flow (%d fields on %s) and ground truth (%d fields on %s) differ" % (nf, dev, n, gt.device))
    if mode not in (0, 1):
        raise RuntimeError("mode must be 0 (every pixel) or 1 (known, non-zero ground truth), got %r" % (mode,))
    g = gt.contiguous()
    lib = hb.load()
    with torch.cuda.device(dev):
        nbytes = lib.ssm_flow_metrics_workspace_bytes(n, h, w)
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        sums = torch.empty(n, 3, dtype=torch.float64, device=dev)
        hb.check(lib.ssm_flow_metrics_fwd(view, g.data_ptr(), n, h, w, top, left, mode, ws.data_ptr(), nbytes, sums.data_ptr(),
                                          hb.stream_ptr()))
    return sums


def metrics_from_flow_sums(sums, h=None, w=None):
    """[N,3] float64 sums -> [N,2] float64 (EPE, share of pixels more than 3 px off); NaN where no pixel counted.  With h, w (mode 0:
    every pixel counts) the share is formed as compute_metrics forms it, count / h / w, so it equals the reference's bit for bit."""
    sums = np.asarray(sums, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        share = sums[:, 1] / sums[:, 2] if h is None else sums[:, 1] / h / w
        return np.stack([sums[:, 0] / sums[:, 2], share], axis=1)


def flow_metrics(flow, gt, top=0, left=0, mode=0):
    """compute_metrics per field on the GPU: host float64 array [N,2] of (EPE, share of pixels more than 3 px off)."""
    sums = flow_metric_sums(flow, gt, top, left, mode).cpu().numpy()
    return metrics_from_flow_sums(sums, *((gt.shape[1], gt.shape[2]) if mode == 0 else ()))


def flow_to_rgb(flow, h, w, top=0, left=0):
    """flo_utils.flow_to_image per field on the GPU (ssm_flow_to_rgb_fwd): the h x w crop at (top, left) of a [N,2,*,*] flow
    (tensor or PlaneChannels) -> uint8 [N,h,w,3] RGB on the device.  Launched on the current stream; no synchronisation."""
    view, n, dev, keep = _field(flow, h, w, top, left)
    lib = hb.load()
    with torch.cuda.device(dev):
        nbytes = lib.ssm_flow_to_rgb_workspace_bytes(n, h, w)
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        rgb = torch.empty(n, h, w, 3, dtype=torch.uint8, device=dev)
        hb.check(lib.ssm_flow_to_rgb_fwd(view, rgb.data_ptr(), n, h, w, top, left, ws.data_ptr(), nbytes, hb.stream_ptr()))
    return rgb


# ---- forward-backward consistency of a pair's two flows (include/ssm_hip.h: ssm_flow_consistency_fwd) -------------------------------------
# alpha and beta: the numbers of Sundaram, Brox and Keutzer (2010) as most later work uses them.  A convention, NOT backed by a measurement
# here - and with this repository's synthetic weights the scores say nothing about quality.
FLOW_ALPHA, FLOW_BETA = 0.01, 0.5
CONSISTENT, INCONSISTENT, LEAVES = 0, 1, 2          # the mask's codes


class FlowCheck(namedtuple("FlowCheck", "judged inconsistent leaves residual_sum")):
    """One pair's record of ssm_flow_consistency_fwd / flow_consistency_host: per direction (0: F01 followed, F10 sampled; 1: the roles
    swapped) the pixels judged (they do not leave the crop), those of them that are inconsistent, the pixels that leave, and the fp64 sum
    of the judged pixels' residuals.  The counts are integers and every share a Fraction: the verdict of a threshold depends on no rounding."""
    __slots__ = ()

    @classmethod
    def of(cls, record):
        """record: [2][4] float64 of one pair, as the entry point writes it."""
        r = np.asarray(record, dtype=np.float64).reshape(2, 4)
        return cls(*(tuple(int(r[d, m]) for d in (0, 1)) for m in range(3)), tuple(float(r[d, 3]) for d in (0, 1)))

    def share(self, d):
        """Inconsistent among the judged pixels of direction d; 1 when nothing was judged - a field that leaves everywhere vouches for nothing."""
        return Fraction(self.inconsistent[d], self.judged[d]) if self.judged[d] else Fraction(1)

    @property
    def score(self):
        return max(self.share(0), self.share(1))

    @property
    def mean_residual(self):
        """The mean residual, in pixels, over the judged pixels of both directions; 0.0 when nothing was judged."""
        n = self.judged[0] + self.judged[1]
        return (self.residual_sum[0] + self.residual_sum[1]) / n if n else 0.0


def flow_consistency_host(flow4, top, left, H, W, alpha=FLOW_ALPHA, beta=FLOW_BETA):
    """The numpy float32 yardstick of ssm_flow_consistency_fwd, op for op the definition of include/ssm_hip.h: flow4 [N,4,*,*] float32
    (F01.u | F01.v | F10.u | F10.v) cropped at (top, left) to H x W -> (record float64 [N,2,4] = judged, inconsistent, leaves, fp64 sum
    of the judged residuals per direction; mask uint8 [N,2,H,W] = 0 consistent, 1 inconsistent, 2 leaves).  Nothing outside the crop is read."""
    f32 = np.float32
    flow4 = np.asarray(flow4, dtype=f32)
    assert flow4.ndim == 4 and flow4.shape[1] == 4, "flow4 must be [N,4,*,*]; got %s" % (flow4.shape,)
    assert H >= 1 and W >= 1 and top >= 0 and left >= 0 and top + H <= flow4.shape[2] and left + W <= flow4.shape[3], \
        "crop %dx%d at (%d, %d) does not fit the %dx%d flow" % (H, W, top, left, flow4.shape[2], flow4.shape[3])
    crop = flow4[:, :, top:top + H, left:left + W]
    n = crop.shape[0]
    alpha, beta = f32(alpha), f32(beta)
    xs, ys = np.arange(W, dtype=f32)[None, None, :], np.arange(H, dtype=f32)[None, :, None]
    rows = np.arange(n)[:, None, None]
    record, mask = np.zeros((n, 2, 4), np.float64), np.zeros((n, 2, H, W), np.uint8)
    with np.errstate(invalid="ignore", over="ignore"):
        for d in (0, 1):
            u, v = crop[:, 2 * d], crop[:, 2 * d + 1]
            g = crop[:, 2 - 2 * d:4 - 2 * d]
            px, py = xs + u, ys + v
            leaves = ~((px >= 0) & (px <= f32(W - 1)) & (py >= 0) & (py <= f32(H - 1)))
            px, py = np.where(leaves, f32(0), px), np.where(leaves, f32(0), py)          # a pixel that leaves takes no tap
            x0, y0 = np.floor(px), np.floor(py)
            fx, fy = px - x0, py - y0
            xi0, yi0 = x0.astype(np.int64), y0.astype(np.int64)
            xi1, yi1 = np.minimum(xi0 + 1, W - 1), np.minimum(yi0 + 1, H - 1)
            s = []
            for c in (0, 1):
                gc = g[:, c]
                g00, g01, g10, g11 = gc[rows, yi0, xi0], gc[rows, yi0, xi1], gc[rows, yi1, xi0], gc[rows, yi1, xi1]
                a = g00 + fx * (g01 - g00)
                b = g10 + fx * (g11 - g10)
                s.append(a + fy * (b - a))
            rx, ry = u + s[0], v + s[1]
            e2 = rx * rx + ry * ry
            m2 = ((u * u + v * v) + s[0] * s[0]) + s[1] * s[1]
            bad = ~leaves & (e2 > alpha * m2 + beta)
            residual = np.sqrt(e2)
            assert residual.dtype == f32
            mask[:, d] = np.where(leaves, LEAVES, np.where(bad, INCONSISTENT, CONSISTENT))
            record[:, d, 0] = (~leaves).reshape(n, -1).sum(axis=1)
            record[:, d, 1] = bad.reshape(n, -1).sum(axis=1)
            record[:, d, 2] = leaves.reshape(n, -1).sum(axis=1)
            record[:, d, 3] = np.where(leaves, 0.0, residual.astype(np.float64)).reshape(n, -1).sum(axis=1)
    return record, mask


def flow_consistency(flow, h, w, top=0, left=0, alpha=FLOW_ALPHA, beta=FLOW_BETA, want_mask=False, out=None, workspace=None):
    """ssm_flow_consistency_fwd on the h x w crop at (top, left) of a [N,4,*,*] flow - a float32 device tensor with unit x-stride, or the
    4-channel hipbind.Planes stage 1 leaves (FullModel.estimate_flow(..., want_planes=True), PairEngine.s1.t["out"]) -> float64 [N,2,4]
    on the device (into `out` if given), FlowCheck.of(row) on the host; with want_mask (True, or the caller's own contiguous uint8
    [N,2,h,w] device tensor to write it into) (record, uint8 [N,2,h,w] mask).  workspace: a
    uint8 device tensor of ssm_flow_consistency_workspace_bytes(N, h, w) bytes at least, the caller's (a loop that allocates nothing);
    None: made here.  Launched on the current stream; no synchronisation."""
    if isinstance(flow, hb.Planes):
        view, shape, dev, keep = flow.view(), (flow.B, flow.C, flow.H, flow.W), flow.buf.device, flow
    else:
        if not (isinstance(flow, torch.Tensor) and flow.is_cuda and flow.dtype == torch.float32 and flow.dim() == 4):
            raise RuntimeError("flow must be a [N,4,H,W] float32 tensor on the GPU (or hipbind.Planes); got %s %s on %s"
                               % (getattr(flow, "dtype", type(flow)), tuple(getattr(flow, "shape", ())), getattr(flow, "device", "?")))
        keep = flow if flow.stride(3) == 1 else flow.contiguous()
        view, shape, dev = hb.view_of(keep), tuple(keep.shape), keep.device
    if shape[1] != 4:
        raise RuntimeError("flow must hold the four planes F01 | F10; got %d channels" % shape[1])
    if not (h >= 1 and w >= 1 and top >= 0 and left >= 0 and top + h <= shape[2] and left + w <= shape[3]):
        raise RuntimeError("crop %dx%d at (%d, %d) does not fit the %dx%d flow" % (h, w, top, left, shape[2], shape[3]))
    n = shape[0]
    lib = hb.load()
    with torch.cuda.device(dev):
        nbytes = lib.ssm_flow_consistency_workspace_bytes(n, h, w)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if workspace is None else workspace
        assert ws.is_cuda and ws.dtype == torch.uint8 and ws.is_contiguous() and ws.numel() >= nbytes, "workspace of %d bytes needed" % nbytes
        if out is None:
            out = torch.empty(n, 2, 4, dtype=torch.float64, device=dev)
        assert out.is_cuda and out.dtype == torch.float64 and tuple(out.shape) == (n, 2, 4) and out.is_contiguous()
        if isinstance(want_mask, torch.Tensor):          # the caller's own mask, as `out` and `workspace` are the caller's
            mask = want_mask
            assert mask.is_cuda and mask.dtype == torch.uint8 and tuple(mask.shape) == (n, 2, h, w) and mask.is_contiguous()
        else:
            mask = torch.empty(n, 2, h, w, dtype=torch.uint8, device=dev) if want_mask else None
        hb.check(lib.ssm_flow_consistency_fwd(view, n, h, w, top, left, float(alpha), float(beta), ws.data_ptr(), out.data_ptr(),
                                              None if mask is None else mask.data_ptr(), hb.stream_ptr()))
    return (out, mask) if mask is not None else out


def parse_flow_check(value, alpha=None, beta=None):
    """The option flow_check -> (T or None, alpha or None, beta or None), exact Fractions: True is the report alone; a threshold is "T"
    or "T:ALPHA:BETA" (or a number, a Fraction, or such a triple), each written as a decimal or a fraction, T >= 0 (a pair falls back
    iff its score >= T; scores lie in [0, 1], so T = 0 condemns every pair and any T > 1 none), ALPHA and BETA >= 0.  alpha, beta: the
    same numbers given on their own, which go before the triple's.  There is no default T, and None for alpha or beta means the
    convention FLOW_ALPHA, FLOW_BETA.  Anything else is a ValueError naming the value."""
    parts = [] if value is True else (value.strip().split(":") if isinstance(value, str) else (
        list(value) if isinstance(value, (tuple, list)) else [value]))
    if len(parts) not in (0, 1, 3) or any(p is None or isinstance(p, bool) for p in parts):
        raise ValueError("a flow check is written T or T:ALPHA:BETA, e.g. 0.2 or 1/5:0.01:0.5 (got %r)" % (value,))
    parts = (parts + [None] * 3)[:3]
    parts = [parts[0], parts[1] if alpha is None else alpha, parts[2] if beta is None else beta]
    nums = []
    for name, p in zip(("threshold", "alpha", "beta"), parts):
        try:
            x = None if p is None else Fraction(p.strip() if isinstance(p, str) else p)
        except (ValueError, TypeError, ZeroDivisionError, OverflowError):
            raise ValueError("a flow check's %s is written as a decimal or a fraction, e.g. 0.2 or 1/5 (got %r)" % (name, p)) from None
        if isinstance(p, bool) or (x is not None and x < 0):
            raise ValueError("a flow check's %s is a number that is not negative (got %r)" % (name, p))
        nums.append(x)
    return tuple(nums)


def compute_metrics_host(flow_hw2, gt_hw2):
    """compute_metrics of scripts/evaluate_optical_flow_results.py:18-28 on [1,H,W,2] float32 arrays: (mean end-point error as the
    float32 np.mean of the float32 error map, share of pixels whose error is > 3)."""
    flow_hw2, gt_hw2 = np.asarray(flow_hw2, dtype=np.float32), np.asarray(gt_hw2, dtype=np.float32)
    assert flow_hw2.shape[0] == gt_hw2.shape[0] == 1
    err_map = error_map_host(flow_hw2[0], gt_hw2[0])
    return np.mean(err_map), int((err_map > 3).sum()) / err_map.shape[0] / err_map.shape[1]


def error_map_host(flow_hw2, gt_hw2):
    """The float32 end-point-error map of compute_metrics: sqrt(sum((gt - flow) ** 2, axis=2)), every operation rounded to float32."""
    d = np.asarray(gt_hw2, dtype=np.float32) - np.asarray(flow_hw2, dtype=np.float32)
    return np.sqrt(np.sum(d * d, axis=2, dtype=np.float32))


def sintel_windows(n_images, n_frames=2):
    """`Reader.sliding_window` of scripts/utils/dataloaders/sintel_opticalflow.py:75-93 on indices: windows of N_FRAMES images at step
    1 -> [(input indices, index of the target flow)].  N_FRAMES = 4 pads the index list with one copy at each end; the target flow
    is the window's first index for N_FRAMES = 2 and its second for 4.  A clip shorter than the window yields one window filled with
    None, as more_itertools.windowed does."""
    assert n_frames in (2, 4), "N_FRAMES must be 2 or 4 (sintel_opticalflow.py:34)"
    from .evaluation import _windowed
    idx = list(range(n_images))
    if n_frames == 4:
        idx = [0] + idx
        idx = idx + [idx[-1]]
    return [(list(win), win[0] if n_frames == 2 else win[1]) for win in _windowed(idx, n_frames, 1)]


def clip_flow_samples(frames_u8, flows, cfg=None, n_frames=2):
    """What the Sintel loader yields for one clip (sintel_opticalflow.py:98-131, batch 1): ([1,N,3,Hp,Wp] normalised input,
    [1,H,W,2] ground truth) per window, built on the device from a uint8 clip [L,H,W,3] and its L-1 flows ([L-1,H,W,2] or a
    list): Normalize -> ToTensor -> zero rows in normalised space is one HIP kernel."""
    x = F.frames_from_u8(frames_u8, cfg, pad_before_norm=False)
    for win, target in sintel_windows(frames_u8.shape[0], n_frames):
        assert None not in win, "clip of %d images is too short for N_FRAMES = %d" % (frames_u8.shape[0], n_frames)
        yield x[win][None], torch.as_tensor(flows[target])[None]


class FlowEvaluator:
    """The loop of scripts/evaluate_optical_flow_results.py:38-77 with stage 1 on the HIP path: per sample the stage-1 flow
    (FullModel.estimate_flow - stage 2 never runs), the crop of :63-65 (the centred padding of `frames.padded_dims`; rows 6:442 of
    448 for Sintel), EPE and the share of pixels more than 3 px off, running lists and their means.  `samples`: an iterable of
    ([1,N,3,Hp,Wp] normalised input, [1,H,W,2] ground truth) as the reference's loader yields them (file readers: the script;
    `clip_flow_samples` builds them from a device-resident clip).  metrics="host" copies the cropped flow back and scores it with
    compute_metrics_host (the reference's path); "device" scores it where stage 1 left it (csrc/ssm_flow.hip) and copies [1,3]
    float64 back."""

    def __init__(self, cfg, model, h_in, w_in, metrics="host"):
        assert metrics in ("host", "device"), "metrics must be 'host' or 'device', got %r" % (metrics,)
        self.cfg, self.model, self.metrics = cfg, model, metrics
        self.n_frames = cfg.getint("TRAIN", "N_FRAMES")
        if self.n_frames != 2:
            raise NotImplementedError("N_FRAMES=%d needs the recurrent bottleneck (unpinned upstream); use N_FRAMES=2" % self.n_frames)
        (self.H_REF, self.W_REF), (self.H_START, self.W_START) = F.padded_dims(h_in, w_in)
        self.H_IN, self.W_IN = h_in, w_in
        self.EPE, self.pct_error = [], []

    @torch.no_grad()
    def eval_sample(self, images, gt_flow):
        """images [1,2,3,Hp,Wp] on the device, gt_flow [1,H,W,2] (host or device) -> (EPE, 3-px share) of flowC_01."""
        assert images.shape[0] == 1 and tuple(images.shape[-2:]) == (self.H_REF, self.W_REF), tuple(images.shape)
        assert tuple(gt_flow.shape) == (1, self.H_IN, self.W_IN, 2), tuple(gt_flow.shape)
        top, left, h, w = self.H_START, self.W_START, self.H_IN, self.W_IN
        if self.metrics == "device":
            planes = self.model.estimate_flow(images, want_planes=True)
            gt = torch.as_tensor(gt_flow).to(device=images.device, dtype=torch.float32)
            m = flow_metrics(PlaneChannels(planes, 0), gt, top, left, 0)
            epe, pct = float(m[0, 0]), float(m[0, 1])
        else:
            flow = self.model.estimate_flow(images)
            flow01 = flow[:, 0:2].permute(0, 2, 3, 1)[:, top:top + h, left:left + w].cpu().numpy()
            gt = gt_flow.cpu().numpy() if isinstance(gt_flow, torch.Tensor) else np.asarray(gt_flow)
            epe, pct = compute_metrics_host(flow01, gt)
            epe, pct = float(epe), float(pct)
        self.EPE.append(epe)
        self.pct_error.append(pct)
        return epe, pct

    def means(self):
        return float(np.mean(self.EPE)), float(np.mean(self.pct_error))

    def run_evaluation(self, samples, log=None, total=None):
        """Every sample through eval_sample; with a logger, the reference's "So Far" line every 10 samples (:71-75)."""
        for idx, (images, gt_flow) in enumerate(samples):
            self.eval_sample(images.float(), gt_flow)
            if log is not None and idx % 10 == 0:
                log.info("Iteration: %s of %s" % (idx, total))
                log.info(images.shape)
                log.info(gt_flow.shape)
                log.info("So Far: EPE: %.3f 3_pct_error: %.3f" % self.means())
        epe, pct = self.means()
        return {"EPE": epe, "pct_error": pct, "samples": len(self.EPE)}
