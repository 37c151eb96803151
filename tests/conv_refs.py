"""References for the fp32 FORWARD convolution forms (tests/test_hip_conv_fwd_exact.py, tests/test_hip_conv_fwd_oneterm.py) and the
CPU test of these helpers (tests/test_conv_refs_cpu.py).  A plain helper module (no fixtures, no collection hooks, nothing runs at
import), the way tests/train_refs.py serves the training step.

A. The exact-integer regime.  conv_fwd_exact(x, w, bias, ups=, add=, add_div=, form=) is the float64 evaluation of the oracle's ops
   (oracle.ssm_oracle.conv2d / upsample2x_bilinear) on integer-valued fp32 operands, cast to fp32 - after ASSERTING that fp32 holds
   every value a form can meet on the way exactly, in any summation order (exactness_budget):
       budget = max over outputs of  [ sum |x| |w| + |bias| + |add| ] / granule  <  2^24
   granule: 1 for the direct form; 1/4 for F(2x2,3x3), whose filter transform U = G g G^T, G = [1 0 0; .5 .5 .5; .5 -.5 .5; 0 0 1], has
   entries that are multiples of 1/4; a further 1/16 where the bilinear x2 upsample is fused (weights 0.75 / 0.25 per axis).  For
   F(2x2,3x3) the absolute-value sum is taken through the form itself: |A^T| (sum_c |U| (|B^T| |d| |B|)) |A| - it bounds the 4-term
   sums of B^T d B, every partial sum over the channels of every frequency and the 9-term sums of A^T M A, and it is never below
   the direct form's sum.  Every intermediate is a multiple of the granule below granule * 2^24: fp32 holds it exactly.
   lrelu_once(z): LeakyReLU(0.1) of an exact z with its ONE rounding, fp32(z) * fp32(0.1).
B. One term per output.  sparse_problem(...): activations that are zero except on a lattice of period >= k, one channel per lattice
   pixel, amplitudes +-1, +-2, +-4; the float64 truth of every output is amplitude x tap (+ bias) - no summation, so the error of a
   form is all the form's own (transform constants, cancellation in A^T M A), with nothing of a 4608-term sum to hide in.  With
   ups=True the lattice is the LOW-res source of conv(upsample2x(x)): one low-res pixel of one channel per output, at most k x k terms.
C. fp32 emulations of the Winograd forms, built from Cook-Toom matrices over the points and scalings that the kernels' comments
   document - they share no code with the kernels:
       F(2x2,3x3)               0, +-1, inf;  G rows scaled 1, 1/2, 1/2, 1                                     (csrc/ssm_wino.hip)
       F(4x4,3x3)               0, +-5/8, +-8/5, inf;  monic rows of B^T                                        (csrc/ssm_wino4.hip)
       F(4x4,5x5), F(2,7), F(4,5)   0, +-1, +-2, +-1/2, inf;  c = {1, -2/9, -2/9, 1/90, 1/90, 32/45, 32/45}      (csrc/ssm_wino5_pack.h, ssm_wino1d.hip)
       2x2 blocks of F(4x4,4x4) 0, +-1, +-2, 1/2, inf;  c = {-1/2, -1/3, 1/9, 1/36, -1/60, 32/45}               (csrc/ssm_wino7_pack.h)
   U = G g G^T is evaluated in float64 and rounded once; B^T d B, the sums over channels and A^T M A are fp32, one multiply and one
   add at a time in the matrix steps.  (The matrices of tests/emulate_winograd_*.py, as importable functions.)
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import ssm_oracle as O

TWO24 = 2.0 ** 24
AMPLITUDES = (1.0, -1.0, 2.0, -2.0, 4.0, -4.0)


# ---- A. the exact-integer regime ---------------------------------------------------------------------------------------------------
def int_tensor(shape, gen, lo=-3, hi=3):
    """Integer-valued fp32 tensor, uniform on {lo, ..., hi}."""
    return torch.randint(lo, hi + 1, shape, generator=gen).to(torch.float32)


def lrelu_once(z):
    """What an epilogue must produce from an exact pre-activation: where(z >= 0, z, fp32(z) * fp32(0.1)), one rounding."""
    z = z.to(torch.float32)
    return torch.where(z >= 0, z, z * torch.tensor(0.1, dtype=torch.float32))


def _expand_add(add, add_div, B):
    return None if add is None else add.repeat_interleave(add_div, 0)[:B]


def _granule(ups, form):
    assert form in ("direct", "wino", "upgemm")
    return (1.0 / 16 if ups else 1.0) / (4 if form == "wino" else 1)


def _conv_and_bound(x, w, ups, form):
    """(float64 convolution without bias, the absolute-value sum of module docstring A without bias and addend)."""
    xin, xa = x.double(), x.double().abs()
    if ups:
        xin, xa = O.upsample2x_bilinear(xin), O.upsample2x_bilinear(xa)   # non-negative weights: up(|x|) >= |up(x)| and every partial sum of it
    zero = torch.zeros(w.shape[0], dtype=torch.float64)
    if form == "wino":
        assert w.shape[-1] == 3
        AT, G, BT = f23_matrices()
        bound = winograd_2d(xa, w.double().abs(), None, AT.abs(), G.abs(), BT.abs(), 2, 3, torch.float64)
    else:
        bound = O.conv2d(xa, w.double().abs(), zero)
    return O.conv2d(xin, w.double(), zero), bound


def _with_bias_and_addend(t, bias, add, add_div):
    """t + bias (+ add[b // add_div]) in float64; with the absolute values of bias and addend, the same line extends the bound."""
    t = t + bias.double().view(1, -1, 1, 1)
    return t if add is None else t + _expand_add(add, add_div, t.shape[0]).double()


def _budget(bound, bias, add, add_div, ups, form):
    """(F(2x2,3x3) starts the accumulator of frequency (1, 1) from the bias, which A^T M A adds once to every output: |bias| enters the
    bound once, as in the direct form.)"""
    return float(_with_bias_and_addend(bound, bias.abs(), None if add is None else add.abs(), add_div).max()) / _granule(ups, form)


def _finish_exact(conv, bound, bias, add, add_div, ups, form):
    """bias and addend onto a float64 convolution; the budget and the exact cast, asserted."""
    for t in (bias,) + (() if add is None else (add,)):
        assert t.dtype == torch.float32 and bool((t == t.round()).all()), "integer-valued fp32 operands"
    budget = _budget(bound, bias, add, add_div, ups, form)
    assert budget < TWO24, "the case leaves the exact regime of the %s form: budget %.4g >= 2^24" % (form, budget)
    return exact_f32(_with_bias_and_addend(conv, bias, add, add_div)), budget


def exactness_budget(x, w, bias, ups=False, add=None, add_div=1, form="direct"):
    """The largest [sum of absolute values] / granule any output of the form can meet (module docstring, A); exact while < 2^24."""
    return _budget(_conv_and_bound(x, w, ups, form)[1], bias, add, add_div, ups, form)


def conv_fwd_exact(x, w, bias, *, ups=False, add=None, add_div=1, form="direct"):
    """z = conv(up(x) if ups else x, w) + bias (+ add[b // add_div]) of integer-valued fp32 operands: the float64 oracle cast to fp32,
    which holds it - and every intermediate of `form` - exactly (asserted, never assumed)."""
    for t in (x, w):
        assert t.dtype == torch.float32 and bool((t == t.round()).all()), "integer-valued fp32 operands"
    conv, bound = _conv_and_bound(x, w, ups, form)
    return _finish_exact(conv, bound, bias, add, add_div, ups, form)[0]


def exact_f32(x64):
    """The float64 result cast down, after asserting that fp32 holds it exactly (the comparison is then a bit comparison)."""
    x32 = x64.float()
    assert bool((x32.double() == x64).all()), "the reference left the exact regime"
    return x32


def conv2d_f32_channel_order(x, w, bias, order):
    """fp32 CPU direct convolution summed one input channel at a time in the given channel order (the property the bit tests rest on:
    on operands inside the budget every order gives the same bits)."""
    acc = torch.zeros(x.shape[0], w.shape[0], x.shape[2], x.shape[3], dtype=torch.float32)
    pad = (w.shape[-1] - 1) // 2
    for c in order:
        acc = acc + F.conv2d(x[:, c:c + 1], w[:, c:c + 1], None, padding=pad)
    return acc + bias.view(1, -1, 1, 1)


def pool_bound(y):
    """4 * 2^-24 * sum |y| over each 2x2 block: three adds and one multiply, each rounding once."""
    return 4 * 2.0 ** -24 * O.avg_pool2(y.double().abs()) * 4


# ---- B. one term per output --------------------------------------------------------------------------------------------------------
def sparse_problem(k, cin, cout, B, H, W, period, seed, ups=False):
    """-> (x, w, bias, truth).  x [B,cin,H,W] is zero except on the lattice {(oy + i period, ox + j period)}; the n-th lattice pixel
    (counted over the whole batch) is non-zero in channel (seed + n) % cin only, with amplitude AMPLITUDES[(n + n // cin) % 6]; the
    lattice offset (oy, ox) rotates with the batch entry.  w = randn / sqrt(cin k^2), bias = 0.1 randn.  truth: the float64 convolution -
    with period >= k every output receives at most one product, so it is amplitude x tap + bias with no summation.
    ups: x is the LOW-res source of conv(upsample2x_bilinear(x)), H x W its size, truth the float64 evaluation of that at 2H x 2W.  A
    low-res pixel i feeds the high-res pixels 2i - 1 .. 2i + 2 (weights .25 .75 .75 .25), hence the outputs 2i - 1 - pad .. 2i + 2 + pad: with
    2 period >= k + 3 every output is fed by ONE low-res pixel of one channel (sources_per_output_ups) - a sum of at most k x k terms,
    amplitude x (bilinear weight) x tap, that share the amplitude's sign structure."""
    assert (2 * period >= k + 3) if ups else (period >= k)
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    bias = torch.randn(cout, generator=g) * 0.1
    x = torch.zeros(B, cin, H, W)
    n = 0
    for b in range(B):
        oy, ox = (seed + 2 * b) % period % H, (seed // 3 + 3 * b + 1) % period % W
        for yy in range(oy, H, period):
            for xx in range(ox, W, period):
                x[b, (seed + n) % cin, yy, xx] = AMPLITUDES[(n + n // cin) % len(AMPLITUDES)]
                n += 1
    truth = O.conv2d(O.upsample2x_bilinear(x.double()) if ups else x.double(), w.double(), bias.double())
    return x, w, bias, truth


def terms_per_output(x, k):
    """How many products each output receives: the convolution of the operand's support with a k x k box of ones, channels summed."""
    s = (x != 0).double().sum(1, keepdim=True)
    return F.conv2d(s, torch.ones(1, 1, k, k, dtype=torch.float64), padding=(k - 1) // 2)


def sources_per_output_ups(x, k):
    """How many LOW-res (pixel, channel) entries feed each output of conv_k(upsample2x_bilinear(x)): entry i reaches the outputs
    2i - 1 - pad .. 2i + 2 + pad of either axis (the clamped border rows of the upsample add none) - the operand's support spread by a
    (k + 3) x (k + 3) box at stride 2."""
    s = (x != 0).double().sum(1, keepdim=True)
    return F.conv_transpose2d(s, torch.ones(1, 1, k + 3, k + 3, dtype=torch.float64), stride=2, padding=(k + 1) // 2)


def tile_position_table(err, th=4, tw=4):
    """max |err| per position inside the th x tw output tile: a [th, tw] tensor."""
    e = err.abs()
    return torch.tensor([[float(e[..., i::th, j::tw].max()) if e[..., i::th, j::tw].numel() else 0.0 for j in range(tw)] for i in range(th)])


# ---- C. the Winograd forms in fp32 -------------------------------------------------------------------------------------------------
INF = float("inf")


def cook_toom(m, r, pts, c=None):
    """1-D F(m, r) over the finite points `pts` and the point at infinity: y = AT [(G g) .* (BT d)].  Rows of G are scaled by c (and
    those of BT by 1 / c); c None: the scaling that makes the rows of BT monic (last non-zero coefficient 1).  float64 tensors
    (AT [m, n], G [n, r], BT [n, n]), n = m + r - 1."""
    n = m + r - 1
    assert len(pts) == n - 1

    def V(kk):
        M = np.zeros((n, kk))
        for i, p in enumerate(pts):
            M[i] = [p ** j for j in range(kk)]
        M[n - 1, kk - 1] = 1.0
        return M
    AT, G, BT = V(m).T.copy(), V(r).copy(), np.linalg.inv(V(n)).T.copy()
    for i in range(n):
        f = BT[i][np.abs(BT[i]) > 1e-12][-1] if c is None else (c[i] if i < n - 1 else 1.0)
        BT[i] /= f
        G[i] *= f
    BT[np.abs(BT) < 1e-12] = 0.0
    return tuple(torch.tensor(M, dtype=torch.float64) for M in (AT, G, BT))


def f23_matrices():
    """F(2,3) as csrc/ssm_wino.hip writes it: G = [1 0 0; .5 .5 .5; .5 -.5 .5; 0 0 1], A^T = [1 1 1 0; 0 1 -1 -1], B^T with entries 0, +-1."""
    AT = torch.tensor([[1., 1., 1., 0.], [0., 1., -1., -1.]], dtype=torch.float64)
    G = torch.tensor([[1., 0., 0.], [.5, .5, .5], [.5, -.5, .5], [0., 0., 1.]], dtype=torch.float64)
    BT = torch.tensor([[1., 0., -1., 0.], [0., 1., 1., 0.], [0., -1., 1., 0.], [0., 1., 0., -1.]], dtype=torch.float64)
    return AT, G, BT


C_8PT = (1.0, -2.0 / 9, -2.0 / 9, 1.0 / 90, 1.0 / 90, 32.0 / 45, 32.0 / 45)
C_7PT = (-0.5, -1.0 / 3, 1.0 / 9, 1.0 / 36, -1.0 / 60, 32.0 / 45)
PTS_8 = (0.0, 1.0, -1.0, 2.0, -2.0, 0.5, -0.5)
PTS_7 = (0.0, 1.0, -1.0, 2.0, -2.0, 0.5)
PTS_W4 = (0.0, 0.625, -0.625, 1.6, -1.6)


@functools.lru_cache(maxsize=None)
def form_matrices(form):
    """(m, r, AT, G, BT) of 'wino4' F(4,3), 'wino5' F(4,5), 'wino7' F(4,4) (one block), 'wino1d7' F(2,7), 'wino1d5' F(4,5)."""
    if form == "wino4":
        return (4, 3) + cook_toom(4, 3, PTS_W4)
    if form in ("wino5", "wino1d5"):
        return (4, 5) + cook_toom(4, 5, PTS_8, C_8PT)
    if form == "wino1d7":
        return (2, 7) + cook_toom(2, 7, PTS_8, C_8PT)
    if form == "wino7":
        return (4, 4) + cook_toom(4, 4, PTS_7, C_7PT)
    raise KeyError(form)


def perturbed(G, i, j, rel=1e-5):
    """G with ONE constant changed by `rel` relative (what a constant typed to five digits looks like)."""
    assert float(G[i, j]) != 0.0
    G = G.clone()
    G[i, j] *= 1.0 + rel
    return G


def matapply(Mx, d, dtype):
    """out[i] = sum_j Mx[i, j] d[j] along dim 0 of d: one multiply and one add of `dtype` at a time, zeros skipped, +-1 without a multiply."""
    out = []
    for i in range(Mx.shape[0]):
        acc = None
        for j in range(Mx.shape[1]):
            m = float(Mx[i, j])
            if m == 0.0:
                continue
            t = d[j] if m == 1.0 else (-d[j] if m == -1.0 else torch.tensor(m, dtype=dtype) * d[j])
            acc = t if acc is None else acc + t
        out.append(acc if acc is not None else torch.zeros_like(d[0]))
    return torch.stack(out, 0)


def _windows(x, n, stride, pad, ty, tx):
    """[n, n, B, C, ty, tx]: the n x n input windows at the given stride, zero padding of `pad` before and as much as needed behind."""
    B, C, H, W = x.shape
    xp = F.pad(x, (pad, stride * tx + n - W, pad, stride * ty + n - H))
    win = xp.unfold(2, n, stride).unfold(3, n, stride)[:, :, :ty, :tx]          # [B, C, ty, tx, n, n]
    return win.permute(4, 5, 0, 1, 2, 3).contiguous()


def _filter_transform(w, Gy, Gx, dtype):
    """U[i, j, n, c] = (Gy g Gx^T): float64, rounded ONCE to dtype."""
    return torch.einsum("ik,nckl,jl->ijnc", Gy, w.double(), Gx).to(dtype)


def winograd_2d(x, w, bias, AT, G, BT, m, r, dtype):
    """'same' convolution as F(m x m, r x r) in `dtype` (float64: the algebra; float32: the emulation)."""
    B, C, H, W = x.shape
    n = m + r - 1
    ty, tx = -(-H // m), -(-W // m)
    U = _filter_transform(w, G, G, dtype)
    d = _windows(x.to(dtype), n, m, (r - 1) // 2, ty, tx)
    V = matapply(BT, d, dtype)                                  # rows
    V = matapply(BT, V.transpose(0, 1), dtype).transpose(0, 1)  # columns
    M = torch.einsum("ijnc,ijbcyx->ijbnyx", U, V)
    return _output_transform(M, AT, AT, m, m, H, W, bias, dtype)


def _output_transform(M, ATy, ATx, my, mx, H, W, bias, dtype):
    Y = matapply(ATy, M, dtype)
    Y = matapply(ATx, Y.transpose(0, 1), dtype).transpose(0, 1)          # [my, mx, B, N, ty, tx]
    _, _, B, N, ty, tx = Y.shape
    y = Y.permute(2, 3, 4, 0, 5, 1).reshape(B, N, ty * my, tx * mx)[:, :, :H, :W]
    return y if bias is None else y + bias.to(dtype).view(1, -1, 1, 1)


def emulate_2d(form, x, w, bias, dtype=torch.float32, G=None):
    """'wino4' / 'wino5': the two-dimensional forms.  G: a replacement filter-transform matrix (the perturbed-constant check)."""
    m, r, AT, G0, BT = form_matrices(form)
    assert w.shape[-1] == r
    return winograd_2d(x, w, bias, AT, G0 if G is None else G, BT, m, r, dtype)


def emulate_wino7(x, w, bias, dtype=torch.float32, G=None):
    """The 7x7 filter padded to 8x8 and cut into 2x2 blocks of 4x4 taps, each a F(4x4,4x4) filter: windows of 7 at stride 4, the four
    blocks read the windows at tile offsets (by, bx), summed with the channels in the transform domain."""
    m, r, AT, G0, BT = form_matrices("wino7")
    G = G0 if G is None else G
    B, C, H, W = x.shape
    ty, tx = -(-H // 4), -(-W // 4)
    d = _windows(x.to(dtype), 7, 4, 3, ty + 1, tx + 1)
    V = matapply(BT, d, dtype)
    V = matapply(BT, V.transpose(0, 1), dtype).transpose(0, 1)
    w8 = F.pad(w.double(), (0, 1, 0, 1))
    M = torch.zeros(7, 7, B, w.shape[0], ty, tx, dtype=dtype)
    for by in range(2):
        for bx in range(2):
            U = _filter_transform(w8[:, :, 4 * by:4 * by + 4, 4 * bx:4 * bx + 4], G, G, dtype)
            M = M + torch.einsum("ijnc,ijbcyx->ijbnyx", U, V[:, :, :, :, by:by + ty, bx:bx + tx])
    return _output_transform(M, AT, AT, 4, 4, H, W, bias, dtype)


def emulate_wino1d(x, w, bias, dtype=torch.float32, G=None):
    """F(2,7) / F(4,5) along x, the rows of the filter summed with the channels in the transform domain (csrc/ssm_wino1d.hip)."""
    k = w.shape[-1]
    m, r, AT, G0, BT = form_matrices("wino1d%d" % k)
    G = G0 if G is None else G
    B, C, H, W = x.shape
    n, pad = m + r - 1, (r - 1) // 2
    tx = -(-W // m)
    U = torch.einsum("fk,ncyk->fync", G, w.double()).to(dtype)          # [n, ky, N, C]
    xp = F.pad(x.to(dtype), (pad, m * tx + n - W, pad, pad))
    d = torch.stack([xp[:, :, :, j:j + m * tx:m] for j in range(n)], 0)          # [n, B, C, H + 2 pad, tx]
    V = matapply(BT, d, dtype)
    M = torch.zeros(n, B, w.shape[0], H, tx, dtype=dtype)
    for ky in range(k):
        M = M + torch.einsum("fnc,fbchx->fbnhx", U[:, ky], V[:, :, :, ky:ky + H])
    Y = matapply(AT, M, dtype)                                           # [m, B, N, H, tx]
    y = Y.permute(1, 2, 3, 4, 0).reshape(B, w.shape[0], H, tx * m)[:, :, :, :W]
    return y + bias.to(dtype).view(1, -1, 1, 1)


EMULATIONS = {"wino4": functools.partial(emulate_2d, "wino4"), "wino5": functools.partial(emulate_2d, "wino5"), "wino7": emulate_wino7,
              "wino1d": emulate_wino1d}
ONETERM_MARGIN = 4.0          # summation order over the 36 - 64 frequencies and FMA contraction: neither changes the order of magnitude
ONETERM_FLOOR_ROUNDINGS = 4.0          # the bar never drops below this many roundings (2^-24 relative each) of the largest output


def emulation_error(form, x, w, bias, truth, G=None):
    """(max, rms) error of the fp32 emulation of `form` against the float64 truth."""
    e = EMULATIONS[form](x, w, bias, torch.float32, G=G).double() - truth
    return float(e.abs().max()), float(e.pow(2).mean().sqrt())


def oneterm_bar(emax, truth):
    """The bar of tests/test_hip_conv_fwd_oneterm.py: ONETERM_MARGIN x the largest error `emax` of the emulation on the very same operands.
    On a map with a handful of lattice pixels that largest error can be a single rounding of one output (or, by luck, nothing), which says
    nothing about another summation order: the bar is floored at ONETERM_FLOOR_ROUNDINGS x 2^-24 x max |truth| - the last steps of any form
    (the final adds of A^T M A, the bias) round at the output's magnitude at least that often.  The floor is 2.4e-7 at unit output scale,
    below every 4 x emulation figure of the several-tile maps."""
    return max(ONETERM_MARGIN * emax, ONETERM_FLOOR_ROUNDINGS * 2.0 ** -24 * float(truth.abs().max()))


def filter_transform_matrix(form, k=None):
    """G of a form ('wino1d': of its F(2,7) for k = 7, of its F(4,5) for k = 5)."""
    return form_matrices("wino1d%d" % k if form == "wino1d" else form)[3]


# ---- packed filters (tests/test_hip_conv_fwd_oneterm.py) -----------------------------------------------------------------------------
def packed_wino5_reference(w):
    """float64 U = G g G^T in the layout of csrc/ssm_wino5_pack.h: [Cout/32][CinP/4][16 quads][4 channels][32 couts][4]; quad 2 rf + h
    holds the column frequencies {0, 1, 2, 7} (h = 0) / {3, 4, 5, 6} (h = 1) of row frequency rf; zero beyond Cout and Cin."""
    cout, cin = w.shape[:2]
    G = form_matrices("wino5")[3]
    U = torch.einsum("ik,nckl,jl->ncij", G, w.double(), G)
    nb, ks = -(-cout // 32), -(-cin // 4)
    Up = torch.zeros(nb * 32, ks * 4, 8, 8, dtype=torch.float64)
    Up[:cout, :cin] = U
    cols = torch.tensor([[0, 1, 2, 7], [3, 4, 5, 6]])
    Uq = Up[:, :, :, cols]                                               # [co, ci, rf, h, e]
    Uq = Uq.reshape(nb, 32, ks, 4, 16, 4)                               # [nb, n, ks, cq, fq, e]
    return Uq.permute(0, 2, 4, 3, 1, 5).contiguous()                    # [nb, ks, fq, cq, n, e]


def packed_wino7_reference(w):
    """float64 U_b = G g_b G^T in the layout of csrc/ssm_wino7_pack.h: [Cout/32][Cin][14 quads][4 blocks][32 couts][4]; quad 2 rf + h
    holds the column frequencies 4 h .. 4 h + 3 of row frequency rf, the fourth element of the odd quads is zero."""
    cout, cin = w.shape[:2]
    G = form_matrices("wino7")[3]
    w8 = F.pad(w.double(), (0, 1, 0, 1))
    nb = -(-cout // 32)
    Up = torch.zeros(nb * 32, cin, 4, 7, 8, dtype=torch.float64)        # [co, ci, block, rf, cf (8th: padding)]
    for by in range(2):
        for bx in range(2):
            Up[:cout, :, 2 * by + bx, :, :7] = torch.einsum("ik,nckl,jl->ncij", G, w8[:, :, 4 * by:4 * by + 4, 4 * bx:4 * bx + 4], G)
    Uq = Up.reshape(nb, 32, cin, 4, 14, 4)                              # [nb, n, ci, block, fq, e]
    return Uq.permute(0, 2, 4, 3, 1, 5).contiguous()                    # [nb, ci, fq, block, n, e]


def ulp_distance(got, want64):
    """|got - fp32(want)| in units of the fp32 spacing at fp32(want) (0 where both are exactly zero)."""
    w32 = want64.float()
    spacing = (torch.nextafter(w32.abs(), torch.tensor(INF)) - w32.abs()).double()
    return (got.double() - w32.double()).abs() / spacing


# ---- the case tables of tests/test_hip_conv_fwd_exact.py (budgets asserted on the CPU by tests/test_conv_refs_cpu.py) ------------------
# (B, H, W): tiles overshoot on both axes, maps smaller than a tile, odd sizes, one multi-tile even map; (3, 12, 20): add_div = 3
EXACT_SHAPES = ((2, 22, 44), (1, 23, 40), (3, 6, 2), (1, 9, 131), (1, 5, 7), (1, 1, 1), (2, 32, 64), (3, 12, 20))
EXACT_C1, EXACT_C2, EXACT_COUT, EXACT_COUT_ADD = 16, 8, 40, 128          # cat of two sources; a ragged cout block; whole cout blocks
DEEP_CASES = {3: (512, 128, 2, 22, 22), 5: (64, 64, 2, 22, 22), 7: (32, 32, 2, 22, 22)}          # k: (cin, cout, B, H, W)
FINAL_SHAPES = ((1, 16, 64), (2, 13, 70), (1, 3, 5), (3, 32, 130))          # of test_final_conv_both_forms_vs_oracle
FINAL_NC = (4, 5, 8, 1)


@functools.lru_cache(maxsize=None)
def exact_problem(k, c1, c2, cout, B, H, W, ups=False, bcast=False, form="direct", amp=3, with_add=True):
    """One case of the exact regime, computed once and shared (never modified): sources a [B,c1,.,.] and b [B or 1,c2,.,.] (LOW-res
    H x W when ups), filter, integer bias, integer addends for add_div 1 and (B % 3 == 0) 3, and the exact pre-activations
      z            conv + bias                      z_add[div]   conv + bias + add[b // div]
      lift, z_pos  an integer bias offset and z + lift >= 0: the run in which the fused 2x2 mean is exact."""
    g = torch.Generator().manual_seed(k * 100003 + c1 * 1009 + c2 * 499 + cout * 101 + B * 31 + H * 7 + W + (5 if ups else 0))
    a = int_tensor((B, c1, H, W), g, -amp, amp)
    b = int_tensor((1 if bcast else B, c2, H, W), g, -amp, amp) if c2 else None
    w = int_tensor((cout, c1 + c2, k, k), g, -amp, amp)
    bias = int_tensor((cout,), g, -9, 9)
    x = a if b is None else torch.cat([a, b.expand(B, -1, -1, -1)], 1)
    Ho, Wo = (2 * H, 2 * W) if ups else (H, W)
    p = {"a": a, "b": b, "w": w, "bias": bias, "x": x, "out_hw": (Ho, Wo)}
    conv, bound = _conv_and_bound(x, w, ups, form)
    p["z"], p["budget"] = _finish_exact(conv, bound, bias, None, 1, ups, form)
    p["add"], p["z_add"] = {}, {}
    for div in ((1, 3) if with_add else ()):
        if B % div == 0:
            p["add"][div] = int_tensor((B // div, cout, Ho, Wo), g, -50, 50)
            p["z_add"][div] = _finish_exact(conv, bound, bias, p["add"][div], div, ups, form)[0]
    p["lift"] = float(torch.ceil(-p["z"].min().clamp(max=0)))
    p["z_pos"] = _finish_exact(conv, bound, bias + p["lift"], None, 1, ups, form)[0]
    assert float(p["z_pos"].min()) >= 0
    return p


def exact_case_table():
    """Every (args of exact_problem) that tests/test_hip_conv_fwd_exact.py runs: the strictest form per kernel size (F(2x2,3x3) for 3x3 -
    its budget bounds the direct form's and the low-res GEMM's), so one set of operands serves every form."""
    t = []
    for k in (3, 5, 7):
        form = "wino" if k == 3 else "direct"
        for B, H, W in EXACT_SHAPES:
            t.append((k, EXACT_C1, EXACT_C2, EXACT_COUT, B, H, W, False, False, form))
            t.append((k, EXACT_C1, EXACT_C2, EXACT_COUT_ADD, B, H, W, False, False, form))
        cin, cout, B, H, W = DEEP_CASES[k]
        t.append((k, cin, 0, cout, B, H, W, False, False, form))
    for B, H, W in EXACT_SHAPES:          # fused upsample: LOW-res shapes, second source batch-broadcast, operands on {-2..2}
        t.append((3, EXACT_C1, EXACT_C2, EXACT_COUT, B, H, W, True, True, "wino", 2))
        t.append((3, EXACT_C1, EXACT_C2, EXACT_COUT_ADD, B, H, W, True, True, "wino", 2))
    t.append((3, 256, 0, 128, 2, 11, 11, True, False, "wino", 2))          # deep, fused upsample
    t.append((3, 512, 0, 128, 2, 11, 11, False, False, "wino"))            # the direct form's split-K (odd width)
    t.append((3, 64, 0, 128, 1, 46, 80, False, False, "wino", 3, False))   # F(2x2,3x3) unsplit over 8 chunks, several workgroup tiles
    for nc in FINAL_NC:
        for B, H, W in FINAL_SHAPES:
            t.append((3, 32, 0, nc, B, H, W, False, False, "direct", 3, False))
    return t
