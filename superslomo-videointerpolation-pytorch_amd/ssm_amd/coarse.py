"""Coarse-flow mode (`flow_scale = s`): the two U-Nets run at 1/s of the frame's size, the frame is synthesised at full size.

Beyond the reference's operator surface and an approximation of its output, not parity.  This module holds what the
engine, the tools and the tests share about the mode and needs no GPU:

  check_scale          the accepted scales, refused by name
  size_rule            the frame sizes a scale accepts (multiples of 32*s), refused by name
  upscale_taps         source indices and weights of the map upsampling: the rule csrc/ssm_elem.hip `up_tap` evaluates per lane
  upsample_maps_host   float32 yardstick of the kernel's map sampling: the kernel's operations in the kernel's order
"""
import numpy as np

SCALES = (1, 2, 4)


def check_scale(flow_scale):
    """flow_scale as an int of SCALES; anything else is refused by name."""
    if flow_scale not in SCALES:
        raise ValueError("flow_scale must be 1, 2 or 4 (got %r)" % (flow_scale,))
    return int(flow_scale)


def size_rule(H, W, flow_scale):
    """The U-Nets halve their maps five times, so the low-resolution pass needs multiples of 32 and the frame multiples of 32*s."""
    m = 32 * check_scale(flow_scale)
    assert H % m == 0 and W % m == 0, \
        "flow_scale=%d needs frame sizes that are multiples of 32*flow_scale = %d (got %dx%d)" % (flow_scale, m, H, W)
    return H // flow_scale, W // flow_scale


def upscale_taps(n_lo, s):
    """(i0, i1, lam) for the s*n_lo output indices of one axis: output o reads source samples i0 and i1 with weights 1 - lam and lam.
    The half-pixel rule of F.interpolate(scale_factor=s, mode="bilinear", align_corners=False): position max(0, (o + 0.5)/s - 0.5),
    i0 = floor, i1 = min(i0 + 1, n_lo - 1), lam = position - i0.  For s = 2 and 4 every step is exact in float32 and lam is a multiple
    of 1/8.  int64, int64, float32 arrays."""
    assert s in (2, 4) and n_lo >= 1
    o = np.arange(s * n_lo, dtype=np.float32)
    pos = np.maximum((o + np.float32(0.5)) / np.float32(s) - np.float32(0.5), np.float32(0.0))
    f = np.floor(pos)
    i0 = f.astype(np.int64)
    i1 = np.minimum(i0 + 1, n_lo - 1)
    return i0, i1, (pos - f).astype(np.float32)


def upsample_maps_host(maps, s):
    """[B,C,h,w] float32 (numpy) -> [B,C,s*h,s*w]: bilinear, columns first and then rows, every product and sum rounded to float32 -
    the map sampling of ssm_synthesize_upscaled_fwd, step 2 of its definition (include/ssm_hip.h)."""
    m = np.asarray(maps, dtype=np.float32)
    h, w = m.shape[2:]
    x0, x1, lx = upscale_taps(w, s)
    y0, y1, ly = upscale_taps(h, s)
    one = np.float32(1.0)
    hz = (one - lx) * m[:, :, :, x0] + lx * m[:, :, :, x1]
    ly = ly[None, None, :, None]
    return (one - ly) * hz[:, :, y0] + ly * hz[:, :, y1]
