"""Middlebury optical-flow files, end-point error and colour coding on numpy - the module path and function names of the
reference's scripts/utils/flo_utils.py, restated from its behaviour.  These host functions are the yardsticks the device kernels
of csrc/ssm_flow.hip (ssm_amd.flow_eval) are held to, so every dtype is pinned explicitly and does not drift with numpy's
promotion rules: the error map is float32 (what float32 inputs give in the reference), the colour map float64 (what the
reference's `u / (maxrad + np.finfo(float).eps)` promotes to on numpy >= 2).

Differences from the reference, on purpose: `read_flow` raises on a bad magic number instead of printing and returning None;
the functions do not modify their arguments (the reference zeroes unknown pixels in place); `flow_error` uses a boolean mask
where the reference indexes with a one-element list (flo_utils.py:113), which the numpy used here (2.2.6) refuses ("too many
indices"); no matplotlib (`show_flow`).
"""
import numpy as np

UNKNOWN_FLOW_THRESH = 1e7
FLO_MAGIC = 202021.25


def read_flow(filename):
    """Middlebury .flo -> float32 [h,w,2] (flo_utils.py:40-59): float32 magic 202021.25, int32 w, int32 h, then h*w*2 float32,
    little-endian.  A wrong magic number or a short payload raises ValueError (the reference prints and returns None)."""
    with open(filename, "rb") as f:
        magic = np.frombuffer(f.read(4), dtype="<f4")
        if magic.size != 1 or magic[0] != np.float32(FLO_MAGIC):
            raise ValueError("%s: magic number incorrect, not a .flo file" % filename)
        w, h = (int(v) for v in np.frombuffer(f.read(8), dtype="<i4"))
        data = np.frombuffer(f.read(8 * w * h), dtype="<f4")
    if w < 1 or h < 1 or data.size != 2 * w * h:
        raise ValueError("%s: %d x %d header, %d payload values" % (filename, w, h, data.size))
    return data.reshape(h, w, 2).astype(np.float32)


def flow_bytes(flow):
    """The .flo file of a [h,w,2] flow as a byte string."""
    flow = np.asarray(flow)
    h, w, c = flow.shape
    assert c == 2, c
    return (np.array([FLO_MAGIC], dtype="<f4").tobytes() + np.array([w, h], dtype="<i4").tobytes()
            + np.ascontiguousarray(flow, dtype="<f4").tobytes())


def write_flow(flow, filename):
    """float32 [h,w,2] -> Middlebury .flo (flo_utils.py:63-83)."""
    with open(filename, "wb") as f:
        f.write(flow_bytes(flow))


def flow_error(tu, tv, u, v):
    """Average end-point error over the pixels whose ground truth (tu, tv) is known (|.| <= 1e7 in both components) and not zero
    in both components: the evident definition of flo_utils.py:86-138, in float32.  NaN when no pixel counts."""
    tu, tv, u, v = (np.asarray(a, dtype=np.float32) for a in (tu, tv, u, v))
    unknown = (np.abs(tu) > UNKNOWN_FLOW_THRESH) | (np.abs(tv) > UNKNOWN_FLOW_THRESH)
    counted = ~unknown & ((np.abs(tu) > 0) | (np.abs(tv) > 0))
    du, dv = tu - u, tv - v
    epe = np.sqrt(du * du + dv * dv)
    return np.mean(epe[counted], dtype=np.float32) if counted.any() else np.float32("nan")


def make_color_wheel():
    """The 55 x 3 Middlebury colour wheel (flo_utils.py:225-272), float64: six ramps RY, YG, GC, CB, BM, MR."""
    wheel = np.zeros((55, 3), dtype=np.float64)
    col = 0
    # (length, the channel held at 255, the channel that ramps, ramp falls?)
    for n, full, ramp, falls in ((15, 0, 1, False), (6, 1, 0, True), (4, 1, 2, False), (11, 2, 1, True), (13, 2, 0, False),
                                 (6, 0, 2, True)):
        r = np.floor(255 * np.arange(0, n, dtype=np.float64) / n)
        wheel[col:col + n, full] = 255
        wheel[col:col + n, ramp] = 255 - r if falls else r
        col += n
    return wheel


def compute_color(u, v):
    """Normalised float64 flow components [h,w] -> float64 [h,w,3] of colour levels (flo_utils.py:181-222): angle -> position on the
    wheel, linear interpolation between its two neighbours, saturation by the radius (rad <= 1), * 0.75 beyond; NaN pixels 0."""
    u, v = np.array(u, dtype=np.float64), np.array(v, dtype=np.float64)
    nan = np.isnan(u) | np.isnan(v)
    u[nan] = 0
    v[nan] = 0
    wheel = make_color_wheel()
    ncols = wheel.shape[0]
    rad = np.sqrt(u * u + v * v)
    a = np.arctan2(-v, -u) / np.pi
    fk = (a + 1) / 2 * (ncols - 1) + 1
    k0 = np.floor(fk).astype(int)
    k1 = k0 + 1
    k1[k1 == ncols + 1] = 1
    f = fk - k0
    img = np.zeros(u.shape + (3,), dtype=np.float64)
    inside = rad <= 1
    for i in range(3):
        col0, col1 = wheel[k0 - 1, i] / 255, wheel[k1 - 1, i] / 255
        col = (1 - f) * col0 + f * col1
        col[inside] = 1 - rad[inside] * (1 - col[inside])
        col[~inside] *= 0.75
        img[:, :, i] = np.uint8(np.floor(255 * col * (1 - nan)))
    return img


def flow_to_image(flow):
    """float32 [h,w,2] -> uint8 [h,w,3] in the Middlebury colour code (flo_utils.py:141-178).  Unknown pixels (|u| or |v| > 1e7) are
    flow 0 and black.  The field is divided by its maximum float32 radius + 2^-52 in float64; a field that holds a NaN is divided
    by -1 + 2^-52 instead, as in the reference: np.max is NaN there and Python's max(-1, nan) returns its first argument."""
    flow = np.asarray(flow, dtype=np.float32)
    u, v = flow[:, :, 0].copy(), flow[:, :, 1].copy()
    unknown = (np.abs(u) > UNKNOWN_FLOW_THRESH) | (np.abs(v) > UNKNOWN_FLOW_THRESH)
    u[unknown] = 0
    v[unknown] = 0
    rad = np.sqrt(u * u + v * v)                                  # float32, every operation rounded
    top = np.max(rad) if rad.size else np.float32(-1)
    maxrad = np.float64(top) if top > -1 else np.float64(-1)      # max(-1, np.max(rad)): a NaN maximum fails the comparison
    den = maxrad + np.finfo(np.float64).eps
    img = compute_color(u.astype(np.float64) / den, v.astype(np.float64) / den)
    img[unknown] = 0
    return np.uint8(img)
