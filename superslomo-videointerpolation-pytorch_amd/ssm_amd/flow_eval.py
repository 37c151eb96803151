"""Optical-flow evaluation around the stage-1 pass: what scripts/evaluate_optical_flow_results.py and
scripts/utils/dataloaders/sintel_opticalflow.py do around `FullModel`, restated from their behaviour.

  * `FullModel.estimate_flow` runs stage 1 alone (the reference runs the full model and keeps `intermediate_outputs[0]`);
  * `flow_metrics` / `flow_to_rgb` score and colour-code a flow field on the GPU where stage 1 left it (csrc/ssm_flow.hip);
  * `compute_metrics_host` and scripts/utils/flo_utils.py stay the yardsticks, and `FlowEvaluator(metrics="host")` the default.
"""
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
