"""The plain helpers of the 4:2:2 / 9- to 16-bit video tests (tests/test_video_deep_cpu.py, tests/test_hip_video_deep.py): the formats'
constants and the two conversions as a float64 evaluation written from the defining formulas (Kr / Kb, the code ranges of a bit depth,
interpolation and decimation as matrices from the sample positions) - nothing of it goes through ssm_amd.video.yuv_table - and seeded
inputs.  A plain helper module (no fixtures, no collection hooks), imported as tests/video_clips.py is.
"""
import numpy as np

CENTRED, COSITED, C444, C422 = 0, 1, 2, 3
LIMITED, FULL = 0, 1
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)          # ssm_amd.weights.IMAGENET_MEAN / IMAGENET_STD


def V():
    from ssm_amd import video
    return video


def consts64(matrix, crange, bits):
    """The defining constants of a matrix, a code range and a bit depth, in float64, in code units of that depth."""
    kr, kb = ((0.299, 0.114), (0.2126, 0.0722))[matrix]
    s, peak = float(2 ** (bits - 8)), float(2 ** bits - 1)
    lim = crange == LIMITED
    return dict(kr=kr, kb=kb, kg=1.0 - kr - kb, yspan=219.0 * s if lim else peak, cspan=224.0 * s if lim else peak,
                yoff=16.0 * s if lim else 0.0, coff=128.0 * s, ylo=16.0 * s if lim else 0.0, yhi=235.0 * s if lim else peak,
                clo=16.0 * s if lim else 0.0, chi=240.0 * s if lim else peak)


def dims(h, w, layout):
    """(chroma rows, chroma columns) of a layout."""
    return (h, w) if layout == C444 else ((h, (w + 1) // 2) if layout == C422 else ((h + 1) // 2, (w + 1) // 2))


def planes_of(payload, h, w, layout, bits):
    """[N, frame_bytes] uint8 -> Y, U, V as float64, samples of more than 8 bits read as little-endian 16-bit words."""
    ch, cw = dims(h, w, layout)
    p = payload if bits == 8 else payload.view("<u2")
    n = p.shape[0]
    assert p.shape[1] == h * w + 2 * ch * cw
    return (p[:, :h * w].reshape(n, h, w).astype(np.float64), p[:, h * w:h * w + ch * cw].reshape(n, ch, cw).astype(np.float64),
            p[:, h * w + ch * cw:].reshape(n, ch, cw).astype(np.float64))


def payload_of(y, u, v, bits):
    """Integer planes [N, ., .] -> [N, frame_bytes] uint8."""
    n = y.shape[0]
    p = np.concatenate([y.reshape(n, -1), u.reshape(n, -1), v.reshape(n, -1)], axis=1)
    return p.astype(np.uint8) if bits == 8 else p.astype("<u2").view(np.uint8)


def interp_matrix(n_out, n_in, centred):
    """[n_out, n_in] float64: linear interpolation at the position of output sample x in input units, x/2 - 1/4 (input samples centred
    between two outputs) or x/2 (co-sited with the even outputs), indices clamped to the input."""
    m = np.zeros((n_out, n_in))
    for x in range(n_out):
        pos = x / 2.0 - (0.25 if centred else 0.0)
        i0 = int(np.floor(pos))
        f = pos - i0
        m[x, min(max(i0, 0), n_in - 1)] += 1.0 - f
        m[x, min(max(i0 + 1, 0), n_in - 1)] += f
    return m


def decim_matrix(n_out, n_in, taps):
    """[n_out, n_in] float64: output c = sum_k taps[k] * input[clamp(2c + offset_k)]; taps = {offset: weight}."""
    m = np.zeros((n_out, n_in))
    for c in range(n_out):
        for off, wgt in taps.items():
            m[c, min(max(2 * c + off, 0), n_in - 1)] += wgt
    return m


def rgb64(payload, h, w, layout, matrix, crange, bits):
    """The unclamped R'G'B' of every pixel in 0 .. 255 units, float64: [3][N,h,w]."""
    k = consts64(matrix, crange, bits)
    y, u, v = planes_of(payload, h, w, layout, bits)
    if layout != C444:
        mh = interp_matrix(w, u.shape[2], layout == CENTRED)
        u, v = u @ mh.T, v @ mh.T
        if layout != C422:
            mv = interp_matrix(h, u.shape[1], True)
            u, v = mv @ u, mv @ v
    yl, cb, cr = (y - k["yoff"]) * 255.0 / k["yspan"], (u - k["coff"]) * 255.0 / k["cspan"], (v - k["coff"]) * 255.0 / k["cspan"]
    r = yl + 2.0 * (1.0 - k["kr"]) * cr
    b = yl + 2.0 * (1.0 - k["kb"]) * cb
    g = (yl - k["kr"] * r - k["kb"] * b) / k["kg"]          # from Y = Kr R + Kg G + Kb B
    return r, g, b


def ingest64(payload, h, w, layout, matrix, crange, bits, pad_before_norm=True):
    """The ingest from its definition, float64: [N,3,Hp,Wp]."""
    hp, wp = -(-h // 32) * 32, -(-w // 32) * 32
    top, left = (hp - h) // 2, (wp - w) // 2
    out = np.zeros((payload.shape[0], 3, hp, wp))
    for p, c in enumerate(rgb64(payload, h, w, layout, matrix, crange, bits)):
        if pad_before_norm:
            out[:, p] = (0.0 - MEAN[p]) / STD[p]
        out[:, p, top:top + h, left:left + w] = (np.clip(c, 0.0, 255.0) / 255.0 - MEAN[p]) / STD[p]
    return out


def egress64(x, h, w, layout, matrix, crange, bits):
    """The egress from its definition: (the float64 values BEFORE rounding, in code units, [N, samples]; the codes as a payload)."""
    k = consts64(matrix, crange, bits)
    hp, wp = x.shape[2:]
    top, left = (hp - h) // 2, (wp - w) // 2
    r, g, b = [(x[:, p, top:top + h, left:left + w].astype(np.float64) * STD[p] + MEAN[p]) * 255.0 for p in range(3)]
    yf = k["kr"] * r + k["kg"] * g + k["kb"] * b
    cb, cr = (b - yf) / (2.0 * (1.0 - k["kb"])), (r - yf) / (2.0 * (1.0 - k["kr"]))
    if layout != C444:
        ch, cw = dims(h, w, layout)
        mh = decim_matrix(cw, w, {0: 0.5, 1: 0.5} if layout == CENTRED else {-1: 0.25, 0: 0.5, 1: 0.25})
        cb, cr = cb @ mh.T, cr @ mh.T
        if layout != C422:
            mv = decim_matrix(ch, h, {0: 0.5, 1: 0.5})
            cb, cr = mv @ cb, mv @ cr
    n = x.shape[0]
    pre = np.concatenate([(yf * k["yspan"] / 255.0 + k["yoff"]).reshape(n, -1), (cb * k["cspan"] / 255.0 + k["coff"]).reshape(n, -1),
                          (cr * k["cspan"] / 255.0 + k["coff"]).reshape(n, -1)], 1)
    lo = np.concatenate([np.full(h * w, k["ylo"]), np.full(pre.shape[1] - h * w, k["clo"])])
    hi = np.concatenate([np.full(h * w, k["yhi"]), np.full(pre.shape[1] - h * w, k["chi"])])
    codes = np.clip(np.rint(pre), lo, hi)
    return pre, (codes.astype(np.uint8) if bits == 8 else codes.astype("<u2").view(np.uint8))


def seeded_payload(n, h, w, layout, bits, seed):
    """Random samples over all the codes of the depth, 0 .. 2^bits - 1."""
    ch, cw = dims(h, w, layout)
    rng = np.random.RandomState(seed)
    return payload_of(rng.randint(0, 2 ** bits, size=(n, h * w + 2 * ch * cw)), np.zeros((n, 0)), np.zeros((n, 0)), bits)


SATURATING = ((-1, -1, 1), (1, 1, -1), (1, -1, -1), (-1, 1, 1), (1, 1, 1), (-1, -1, -1))


def seeded_planes(n, h, w, seed, lo=-0.4, hi=1.4):
    """Normalised fp32 planes whose denormalised values cover [lo, hi], with 4 x 4 patches of the six extreme colours inside every crop
    used here: both saturation bounds of every plane are reached whatever the draw."""
    rng = np.random.RandomState(seed)
    hp, wp = -(-h // 32) * 32, -(-w // 32) * 32
    v = rng.uniform(lo, hi, size=(n, 3, hp, wp))
    for i, rgb in enumerate(SATURATING):
        v[:, :, hp // 2 - 2:hp // 2 + 2, wp // 2 - 12 + 4 * i:wp // 2 - 8 + 4 * i] = np.where(np.asarray(rgb) > 0, hi, lo)[None, :, None, None]
    return ((v - np.asarray(MEAN)[None, :, None, None]) / np.asarray(STD)[None, :, None, None]).astype(np.float32)


def ramp_payload(h, w, layout, crange, bits, seed):
    """Three frames of legal codes whose egress values, in exact arithmetic, are whole numbers under every layout's filters: frame 0 has
    neutral chroma and luma drawn from all its legal codes, both bounds among them; frames 1 and 2 have luma from the middle 40 % of its range and chroma planes
    that are ramps, c[i][j] = c0 + 64 (a i + b j) with small whole a and b - interpolating such a plane (weights in sixteenths) and
    decimating it again (weights in quarters) gives multiples of 64 / 64, and every colour stays in gamut, so that no clamp breaks the
    round trip."""
    k = consts64(0, crange, bits)
    ch, cw = dims(h, w, layout)
    rng = np.random.RandomState(seed)
    ylo, yhi, mid = int(k["ylo"]), int(k["yhi"]), int(k["coff"])
    y = np.stack([rng.randint(ylo, yhi + 1, size=(h, w))] + [rng.randint(ylo + 3 * (yhi - ylo) // 10, ylo + 7 * (yhi - ylo) // 10, size=(h, w))
                                                               for _ in range(2)])
    y[0, 0, 0], y[0, 0, 1] = ylo, yhi          # both bounds of the luma, whatever the draw
    i, j = np.meshgrid(np.arange(ch), np.arange(cw), indexing="ij")
    assert bits == 16, "a ramp of 64 codes per sample stays in gamut only where the codes are many: the 16-bit case"
    u = np.stack([np.full((ch, cw), mid), mid - 300 + 64 * (i + j), mid + 500 - 64 * j])
    v = np.stack([np.full((ch, cw), mid), mid + 700 - 64 * i, mid - 200 + 64 * (2 * i - j)])
    return payload_of(y, u, v, bits)


def ingamut_pixels(count, matrix, crange, bits, seed):
    """`count` random legal (Y, U, V) codes whose unclamped R'G'B' - float64, from the definition - lies in [1, 254]: a 4:4:4 payload of one
    frame of 1 x m pixels, and m."""
    k = consts64(matrix, crange, bits)
    rng = np.random.RandomState(seed)
    y = rng.randint(int(k["ylo"]), int(k["yhi"]) + 1, size=(1, 1, count))
    u = rng.randint(int(k["clo"]), int(k["chi"]) + 1, size=(1, 1, count))
    v = rng.randint(int(k["clo"]), int(k["chi"]) + 1, size=(1, 1, count))
    r, g, b = rgb64(payload_of(y, u, v, bits), 1, count, C444, matrix, crange, bits)
    keep = ((np.minimum(np.minimum(r, g), b) >= 1.0) & (np.maximum(np.maximum(r, g), b) <= 254.0))[0, 0]
    m = int(keep.sum())
    return payload_of(y[:, :, keep], u[:, :, keep], v[:, :, keep], bits), m
