"""Reference evaluation of the coarse-flow synthesis (ssm_synthesize_upscaled_fwd, include/ssm_hip.h) on the CPU, in the dtype
asked for: torch.nn.functional.interpolate for the map upsampling, the oracle's own warp (oracle/ssm_oracle.py, dtype-generic) and the
blend grouped as the oracle's synthesize.  float64 is the yardstick; the float32 evaluation of the SAME expression measures the rounding
the kernel is entitled to (`bar`).  Inputs of the kernel tests are built here as well, so every test of a shape shares one reference."""
import functools

import torch
import torch.nn.functional as F

from oracle import ssm_oracle as O


def synth_upscaled(img6, aux_lo, t, s, dtype=torch.float64):
    """img6 [B or 1,6,H,W], aux_lo [B,5,H/s,W/s] = Ft1 | Ft0 | V0, t [B] -> [B,3,H,W] in `dtype` (CPU)."""
    aux = aux_lo.detach().cpu().to(dtype)
    B = aux.shape[0]
    img = img6.detach().cpu().to(dtype).expand(B, -1, -1, -1)
    tt = t.detach().cpu().to(dtype).view(B, 1, 1, 1)
    up = F.interpolate(aux, scale_factor=s, mode="bilinear", align_corners=False)
    ft1, ft0, v0 = s * up[:, 0:2], s * up[:, 2:4], up[:, 4:5]
    v1 = 1 - v0
    p0 = v0 * O.warp(img[:, 0:3].contiguous(), ft0)
    p1 = v1 * O.warp(img[:, 3:6].contiguous(), ft1)
    return ((1 - tt) * p0 + tt * p1) / ((1 - tt) * v0 + tt * v1)


def bar(img6, aux_lo, t, s):
    """(float64 reference, d, bound): d = max |float32 evaluation - float64| of the expression above on these inputs, bound =
    max(4 d, 1e-6).  The kernel performs the same rounded operations as the float32 evaluation; the factor covers another, equally valid
    order inside the bilinear sums, the floor inputs whose d happens to be tiny."""
    want = synth_upscaled(img6, aux_lo, t, s, torch.float64)
    d = (synth_upscaled(img6, aux_lo, t, s, torch.float32).double() - want).abs().max().item()
    return want, d, max(4.0 * d, 1e-6)


FAMILIES = ("small", "outside")


@functools.lru_cache(maxsize=None)
def kernel_case(h, w, s, family, B=3):
    """Inputs of one kernel test and their reference, computed once: random full-size frames [B,6,s*h,s*w], visibility in (0.05, 0.95)
    (so the denominator (1-t) v0 + t v1 stays above 0.05 for every t in (0,1)), distinct t per entry, and low-resolution flows of
      "small"    a few pixels: +-3 low-resolution pixels
      "outside"  up to +-(size + 2) low-resolution pixels per axis: the scaled flows carry the samples beyond every side of the frame.
    Returns a dict of CPU float32 tensors plus want (float64), d and bound for the per-entry and the batch-broadcast (entry 0's frames)
    forms."""
    assert family in FAMILIES
    g = torch.Generator().manual_seed(1000 * h + 10 * w + s + (7 if family == "outside" else 0))
    H, W = s * h, s * w
    img6 = torch.randn(B, 6, H, W, generator=g)
    u = torch.rand(B, 5, h, w, generator=g)
    aux = torch.empty(B, 5, h, w)
    if family == "small":
        aux[:, 0:4] = 6.0 * u[:, 0:4] - 3.0
    else:
        amp = torch.tensor([w + 2.0, h + 2.0, w + 2.0, h + 2.0]).view(1, 4, 1, 1)
        aux[:, 0:4] = (2.0 * u[:, 0:4] - 1.0) * amp
    aux[:, 4] = 0.05 + 0.9 * u[:, 4]
    t = torch.tensor([0.25, 0.5, 0.8125][:B] if B <= 3 else [(i + 1.0) / (B + 1.0) for i in range(B)])
    case = {"img6": img6, "aux": aux, "t": t, "s": s, "H": H, "W": W}
    case["each"] = bar(img6, aux, t, s)
    case["bcast"] = bar(img6[:1], aux, t, s)
    return case
