"""Float64 references for the element-wise kernels of the training step (csrc/ssm_bwd.hip, csrc/ssm_rnn.hip) and of the inference
path (the forward kernels of csrc/ssm_elem.hip: tests/test_hip_infer_elementwise.py), and the plain helpers both GPU modules share.

A plain helper module (no fixtures, no collection hooks).  Everything here is the CPU oracle (oracle/ssm_oracle.py) evaluated
under torch.autograd in the dtype asked for: O.warp, O.flow_interp_inputs, O.synthesize, O.upsample2x_bilinear and O.avg_pool2
take float64 tensors as they stand.  The recurrent cells are the formulas of O.convlstm_cell / O.convgru_cell without their
convolutions (the kernels take the summed pre-activations).

The last section serves tests/test_hip_wgrad_exact.py: integer-valued inputs and the weight gradient they give exactly.

Inputs are always DRAWN in fp32 and cast up, so the kernel under test and the float64 reference see the same numbers.

Tolerances (tests/test_hip_train_elementwise.py, tests/test_hip_infer_elementwise.py): err <= bar(e_ref) = max(8 * e_ref, 4 * 2**-24), where err is the largest
error over the kept entries relative to the largest reference entry and e_ref = ref_gap(...) is the fp32 CPU oracle's own
distance from the float64 oracle on the same inputs - never a figure of the code under test.
"""
import torch

from oracle import ssm_oracle as O

COORD_WINDOW = 1e-4     # px: a sampling coordinate this close to an integer may floor() differently in fp32 and float64
L1_WINDOW = 1e-5        # an L1 argument this small may take a different sign() in fp32 and float64
ULP4 = 4 * 2.0 ** -24   # four fp32 unit roundoffs: expf / division / tanhf of the device vs libm, one each, where e_ref ~ 0

# (B, H, W), flow scale: the smallest shapes that exercise each indexing decision of the 64 x 4 pixel blocks
SAMPLER_CASES = (
    ((2, 20, 28), 2.0),      # the shape tests/test_hip_backward.py already runs
    ((3, 9, 70), 3.0),       # second 64-wide block column, ragged 4-row block, three distinct t / c_rec / c_warp
    ((1, 4, 64), 2.0),       # exactly one block
    ((1, 5, 65), 2.0),       # one pixel past the block on both axes
    ((2, 1, 5), 1.0),        # H = 1: the max(H - 1, 1) normalisation
    ((1, 37, 1), 1.0),       # W = 1: the max(W - 1, 1) normalisation
    ((2, 5, 3), 6.0),        # most taps outside the image
)
# sizes for the loss sums only: H * W below the 64 chunks (some chunks empty), H * W no multiple of 64
LOSS_ONLY_CASES = (((2, 3, 5), 1.0), ((1, 7, 19), 2.0))
SEED = 11
NAN = float("nan")


def bar(e_ref, ratio=8.0):
    return max(ratio * e_ref, ULP4)


def make_case(shape, flow_scale, seed=SEED):
    """fp32 inputs of one sampler / loss case (the distributions of tests/test_hip_backward.py's case, any shape)."""
    B, H, W = shape
    g = torch.Generator().manual_seed(seed)
    c = {
        "img6": torch.randn(B, 6, H, W, generator=g),
        "flow4": torch.randn(B, 4, H, W, generator=g) * flow_scale,
        "out5": torch.randn(B, 5, H, W, generator=g) * 1.5,
        "target": torch.randn(B, 3, H, W, generator=g),
        "r16": torch.randn(B, 16, H, W, generator=g) * 0.01,
        "dy_extra": torch.randn(B, 3, H, W, generator=g) * 0.5,
        "t": torch.tensor([0.25, 0.625, 0.875])[:B].clone(),
        "c_rec": torch.tensor([0.7, 1.3, 0.2])[:B].clone(),
        "c_warp": torch.tensor([0.4, 0.9, 1.6])[:B].clone(),
    }
    return c


def _per(z):
    return z.abs().flatten(1).sum(1)


def loss_and_grads(img6, flow4, out5, target, t, c_rec, c_warp, r16, dy_extra, s1_terms, s2_terms, dtype=torch.float64):
    """The scalar  sum_b [ c_rec |pred - I_t|_1 + c_warp (enabled warp terms) ] + <in16, r16> + <pred, dy_extra>  and everything
    the kernels are held to.  Returns a dict:
      sums    [B,2]  sum |pred - target|, sum of the enabled warp maps          (what ssm_train_loss_sums returns)
      dout5, dflow4  gradients wrt stage 2's output and stage 1's flows        (ssm_synthesize_bwd + ssm_flowinterp_inputs_bwd)
      in16, pred     forward values (est4 = in16[:, 6:10])
      flows          every flow a sampler used: Ft1^, Ft0^, refined Ft1, Ft0, then F01, F10 if s1_terms
      l1_args        every tensor an abs() was taken of
    """
    c = lambda z: None if z is None else z.detach().to(dtype)     # noqa: E731
    img6, target, r16, dy_extra, c_rec, c_warp = c(img6), c(target), c(r16), c(dy_extra), c(c_rec), c(c_warp)
    B = img6.shape[0]
    tt = c(t).view(B, 1, 1, 1)
    flow4, out5 = c(flow4).requires_grad_(), c(out5).requires_grad_()
    in16 = O.flow_interp_inputs(img6, flow4, tt)
    pred = O.synthesize(img6, in16, out5, tt)
    i0, i1 = img6[:, 0:3], img6[:, 3:6]
    ft1, ft0 = in16[:, 6:8] + out5[:, 1:3], in16[:, 8:10] + out5[:, 3:5]
    l1 = [pred - target]
    flows = [in16[:, 6:8], in16[:, 8:10], ft1, ft0]
    rec = _per(l1[0])
    loss = (c_rec * rec).sum()
    if r16 is not None:
        loss = loss + (in16 * r16).sum()
    if dy_extra is not None:
        loss = loss + (pred * dy_extra).sum()
    wrp = torch.zeros(B, dtype=dtype)
    if s2_terms:
        l1 += [O.warp(i0, ft0) - target, O.warp(i1, ft1) - target]
        wrp = wrp + _per(l1[-2]) + _per(l1[-1])
    if s1_terms:
        flows += [flow4[:, 0:2], flow4[:, 2:4]]
        l1 += [O.warp(i1, flow4[:, 0:2]) - i0, O.warp(i0, flow4[:, 2:4]) - i1]
        wrp = wrp + _per(l1[-2]) + _per(l1[-1])
    loss = loss + (c_warp * wrp).sum()
    loss.backward()
    return {"sums": torch.stack([rec, wrp], 1).detach(), "dout5": out5.grad, "dflow4": flow4.grad, "in16": in16.detach(),
            "pred": pred.detach(), "flows": [f.detach() for f in flows], "l1_args": [a.detach() for a in l1]}


def warp_grads(img, flow, dy, dtype=torch.float64):
    """Autograd of <O.warp(img, flow), dy>: (dflow, dimg)."""
    img, flow = img.detach().to(dtype).requires_grad_(), flow.detach().to(dtype).requires_grad_()
    (O.warp(img, flow) * dy.to(dtype)).sum().backward()
    return flow.grad, img.grad


def keep_mask(flows, l1_args=()):
    """[B,H,W] bool: pixels at which the loss is smooth enough to compare gradients.  A pixel is dropped when, in the evaluation
    handed in (float64), a sampling coordinate x + u or y + v of any flow lies within COORD_WINDOW of an integer (floor decides the
    taps, and the reference itself rounds coordinates in fp32: O.warp's docstring) or any L1 argument is below L1_WINDOW in
    magnitude (sign decides the gradient).  An axis of size 1 is left out: there the sampling coordinate is 0 * (...) = 0 whatever
    the flow (the max(W - 1, 1) normalisation), the sample does not depend on that flow component and nothing is discontinuous."""
    B, _, H, W = flows[0].shape
    keep = torch.ones(B, H, W, dtype=torch.bool)
    xx = torch.arange(W, dtype=torch.float64).view(1, 1, W)
    yy = torch.arange(H, dtype=torch.float64).view(1, H, 1)
    for f in flows:
        f = f.to(torch.float64)
        for coord, n in ((xx + f[:, 0], W), (yy + f[:, 1], H)):
            if n > 1:
                keep &= (coord - torch.round(coord)).abs() >= COORD_WINDOW
    for a in l1_args:
        keep &= (a.abs() >= L1_WINDOW).all(dim=1)
    return keep


def excluded_share(keep):
    return 1.0 - float(keep.double().mean())


def rel_err(got, want, keep=None):
    """Largest |got - want| over the kept entries, relative to the largest kept reference entry.  keep: [B,H,W] pixels (applied
    to every channel), a mask of want's own shape, or None."""
    got, want = got.detach().to(torch.float64).cpu(), want.detach().to(torch.float64)
    if keep is not None:
        if keep.dim() == want.dim() - 1:
            keep = keep.unsqueeze(1).expand_as(want)
        got, want = got[keep], want[keep]
    if want.numel() == 0:
        return 0.0
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-300))


def ref_gap(fn, keep=None):
    """fn(dtype) -> tensor or tuple of tensors.  The fp32 CPU evaluation's rel_err against the float64 one (one figure per
    tensor): the yardstick of a tolerance."""
    lo, hi = fn(torch.float32), fn(torch.float64)
    if isinstance(hi, torch.Tensor):
        return rel_err(lo, hi, keep)
    return tuple(rel_err(a, b, keep) for a, b in zip(lo, hi))


# ---- recurrent cells without their convolutions (O.convlstm_cell / O.convgru_cell) -----------------------------------------
def lstm_cell(pre, c_prev):
    """pre [B,4*Hc,H,W] = summed pre-activations [i|f|o|g]; c_prev or None (zero state).  Returns (h, c_next)."""
    hc = pre.shape[1] // 4
    i, f, o, g = torch.split(pre, hc, dim=1)
    c_next = torch.sigmoid(i) * torch.tanh(g)
    if c_prev is not None:
        c_next = torch.sigmoid(f) * c_prev + c_next
    return torch.sigmoid(o) * torch.tanh(c_next), c_next


def gru_reset(gates, h_prev):
    """gates [B,2*Hc,H,W] = [gamma|beta]: reset * h, the input of the candidate convolution."""
    hc = gates.shape[1] // 2
    return torch.sigmoid(gates[:, :hc]) * h_prev


def gru_update(gates, cand, h_prev):
    """h' = (1 - update) h + update tanh(cand); h_prev None = zero state."""
    hc = gates.shape[1] // 2
    u = torch.sigmoid(gates[:, hc:])
    out = u * torch.tanh(cand)
    return out if h_prev is None else (1 - u) * h_prev + out


def grads(fn, inputs, cots, dtype):
    """Autograd of sum_k <out_k, cot_k> for fn(*inputs) -> tuple of outputs: (outputs, gradients), inputs that are None skipped
    (their gradient is None)."""
    xs = [None if x is None else x.detach().to(dtype).requires_grad_() for x in inputs]
    outs = fn(*xs)
    outs = outs if isinstance(outs, tuple) else (outs,)
    tot = sum((o * c.to(dtype)).sum() for o, c in zip(outs, cots) if c is not None)
    tot.backward()
    return tuple(o.detach() for o in outs), tuple(None if x is None else (x.grad if x.grad is not None else torch.zeros_like(x)) for x in xs)


# ---- weight gradients in the exact-integer regime (tests/test_hip_wgrad_exact.py) ---------------------------------------------
def int_tensor(shape, gen, lo=-3, hi=3):
    """Integer-valued fp32 tensor, uniform on {lo, ..., hi}."""
    return torch.randint(lo, hi + 1, shape, generator=gen).to(torch.float32)


def conv_wgrad_exact(x, dz, k):
    """(dW, db) of y = conv_kxk(x, w) + b under the upstream gradient dz: float64 CPU autograd of O.conv2d, cast to fp32.  Asserts
    what makes the comparison a bit comparison: the float64 result consists of integers below 2**24, so fp32 holds it - and every
    partial sum of it, in any order - exactly."""
    cout, cin = dz.shape[1], x.shape[1]
    w = torch.zeros(cout, cin, k, k, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    (O.conv2d(x.double(), w, b) * dz.double()).sum().backward()
    for g in (w.grad, b.grad):
        assert bool((g == g.round()).all()) and float(g.abs().max()) < 2.0 ** 24, "the reference left the exact-integer regime"
    bound = 9.0 * x.shape[0] * x.shape[2] * x.shape[3]          # sum over pixels of |dz x|: every partial sum stays below it
    assert bound < 2.0 ** 24 and float(x.abs().max()) <= 3 and float(dz.abs().max()) <= 3
    return w.grad.float(), b.grad.float()


# ---- plain helpers of the GPU modules (tests/test_hip_train_elementwise.py, tests/test_hip_infer_elementwise.py) -------------------
def report(group, case, err, e_ref, share=None):
    print("[elementwise] %-14s %-44s err %.3e  e_ref %.3e  bar %.3e%s"
          % (group, case, err, e_ref, bar(e_ref), "" if share is None else "  excluded %.3f %%" % (100 * share)))


class Box:
    """A [B,C,H,W] fp32 device tensor as plain contiguous NCHW or as padded planes (row stride != W), behind one interface."""

    def __init__(self, hb, dev, layout, x=None, shape=None, fill=NAN):
        self.hb, self.layout = hb, layout
        shape = tuple(x.shape) if x is not None else tuple(shape)
        self.shape = shape
        if layout == "planes":
            self.p = hb.Planes(*shape, dev)
            if x is not None:
                self.p.load(x.to(dev).contiguous())
            else:
                self.p.interior.fill_(fill)
        else:
            self.t = x.to(dev).contiguous().clone() if x is not None else torch.full(shape, fill, device=dev)

    def view(self, c0=0, b0=0):
        if self.layout == "planes":
            return self.p.view(c0=c0, b0=b0)
        return self.hb.view_of(self.t[b0:, c0:])

    def get(self):
        return (self.p.interior if self.layout == "planes" else self.t).cpu()

    def frame_is_zero(self):
        """planes: the kernel wrote the interior only."""
        if self.layout != "planes":
            return True
        f = self.p.full.clone()
        f[:, :, self.hb.SSM_PADY:self.hb.SSM_PADY + self.shape[2], self.hb.SSM_PADX:self.hb.SSM_PADX + self.shape[3]] = 0
        return not bool(f.any())


def dptr(t):
    return t.data_ptr()


def bits(t):
    return t.contiguous().view(torch.int32)


# ---- forward kernels of the inference path (tests/test_hip_infer_elementwise.py) ----------------------------------------------------
LAYOUTS = ("nchw", "planes")
CANARY = -7.5           # written into the tail slack behind the last plane of an output; a kernel must leave it alone
CONSTRUCTED_SHAPES = ((1, 5, 65), (2, 5, 3))     # H - 1 and W - 1 are powers of two: the normalisation round trip is exact in fp32


def plant_canary(box):
    """planes: fill the readable slack behind the last plane of `box` with CANARY."""
    if box.layout == "planes":
        box.p.buf[box.p.full.numel():].fill_(CANARY)
    return box


def canary_intact(box):
    if box.layout != "planes":
        return True
    tail = box.p.buf[box.p.full.numel():]
    return tail.numel() > 0 and bool((bits(tail) == bits(torch.full_like(tail, CANARY))).all())


def warp_fwd(img, flow, dtype=torch.float64):
    return O.warp(img.to(dtype), flow.to(dtype))


def inputs_fwd(img6, flow4, t, dtype=torch.float64):
    """O.flow_interp_inputs: the 16-channel stage-2 input, t [B]."""
    return O.flow_interp_inputs(img6.to(dtype), flow4.to(dtype), t.to(dtype).view(-1, 1, 1, 1))


INPUT_GROUPS = (("I1", 0, 3), ("g(I1)", 3, 6), ("flows", 6, 10), ("g(I0)", 10, 13), ("I0", 13, 16))


def synth_fwd(img6, in16, out5, t, dtype=torch.float64):
    """(y3, Ft1 | Ft0, V0): O.synthesize and the three intermediates ssm_synthesize_fwd writes into `aux`."""
    img6, in16, out5 = img6.to(dtype), in16.to(dtype), out5.to(dtype)
    y3 = O.synthesize(img6, in16, out5, t.to(dtype).view(-1, 1, 1, 1))
    return y3, in16[:, 6:10] + out5[:, 1:5], 1 - torch.sigmoid(out5[:, 0:1])


def saturated_case(shape, flow_scale):
    """make_case with the visibility logit times 40 (|logit| up to ~200): expf(-logit) overflows to inf on one side (V1 = 0), V1 rounds to 1
    on the other (V0 = 0).  t stays inside (0, 1), so the blend's denominator (1 - t) V0 + t V1 is at least min(t, 1 - t) = 0.125."""
    c = make_case(shape, flow_scale)
    c["out5"][:, 0] *= 40.0
    assert bool(((c["t"] > 0) & (c["t"] < 1)).all())
    return c


def sampling_positions(flow, dtype=torch.float32):
    """(ix, iy) [B,H,W]: the sampling position of every pixel, by the steps of O.warp (normalise with max(size - 1, 1), map back)."""
    B, _, H, W = flow.shape
    flow = flow.to(dtype)
    xx = torch.arange(W, dtype=torch.float32).view(1, 1, W).expand(B, H, W)
    yy = torch.arange(H, dtype=torch.float32).view(1, H, 1).expand(B, H, W)
    gx = 2.0 * (xx + flow[:, 0]) / max(W - 1, 1) - 1.0
    gy = 2.0 * (yy + flow[:, 1]) / max(H - 1, 1) - 1.0
    return ((gx + 1.0) / 2.0) * (W - 1), ((gy + 1.0) / 2.0) * (H - 1)


def _axis_targets(cls, n):
    """cls: int tensor of classes 0..3.  Target coordinates on an axis of n pixels, all multiples of 1/4 of small magnitude:
    0 an integer inside the image; 1 exactly n - 1 (the upper tap is outside, with weight 0); 2 inside (-1, 0) or (n - 1, n) (one tap
    of the axis outside); 3 at or below -1, or at or above n (both taps of the axis outside, or inside with weight 0 at exactly -1).
    The j-th pixel of a class takes the class's j-th variant, cyclically, so six pixels of a class cover all of them."""
    variants = (
        [float(i) for i in range(n)],
        [float(n - 1)],
        [-0.75, n - 1 + 0.25, -0.5, n - 1 + 0.5, -0.25, n - 1 + 0.75],
        [-1.0, float(n), -1.75, n + 0.75, -2.5, n + 1.5],
    )
    flat = cls.flatten()
    out = torch.zeros(flat.shape, dtype=torch.float32)
    for k, vals in enumerate(variants):
        sel = flat == k
        j = torch.cumsum(sel.long(), 0) - 1
        out[sel] = torch.tensor(vals, dtype=torch.float32)[j[sel] % len(vals)]
    return out.view(cls.shape)


def constructed_flow(shape):
    """A flow whose sampling positions are exactly the targets of _axis_targets: u = target - x, built in fp32.  Every combination of
    the four classes on x and y occurs (16 <= B * H * W).  Returns (flow [B,2,H,W], tx, ty, cx, cy), the last four [B,H,W]."""
    B, H, W = shape
    idx = torch.arange(B * H * W).view(B, H, W)
    cx, cy = idx % 4, (idx // 4) % 4
    tx, ty = _axis_targets(cx, W), _axis_targets(cy, H)
    xx = torch.arange(W, dtype=torch.float32).view(1, 1, W)
    yy = torch.arange(H, dtype=torch.float32).view(1, H, 1)
    return torch.stack([tx - xx, ty - yy], 1), tx, ty, cx, cy


# exact-arithmetic kernels: integer-valued inputs, every product with 1/4, 3/4, 1/8 and every sum exact in fp32
AVGPOOL_C = (1, 5, 8, 13)                                    # channel groups of 4: one ragged, one, two whole, three + one
AVGPOOL_HW = ((2, 2), (4, 64), (6, 66), (10, 130))           # input sizes: one output pixel .. a second 64-wide block column
UPSAMPLE_CH = ((3, 2), (4, 0), (8, 8), (5, 0))
UPSAMPLE_HW = ((1, 1), (3, 3), (5, 7), (2, 33), (4, 65), (2, 34))     # low-res; (2, 34): a row's last thread owns a PAIR whose right tap clamps
FINISH_KS = (2, 3, 8)
FINISH_C = (5, 32, 40)
FINISH_HW = ((4, 64), (6, 66), (11, 11), (5, 6))            # (11, 11): the one-pixel kernel; (5, 6): even width, a lone last row
FINISH_SLOPE = 0.125
# name -> (add_div or 0, lrelu, mask, pool, slope)
FINISH_OPTIONS = (
    ("bias-only", 0, False, False, False, FINISH_SLOPE),     # the bias arrives inside partial 0: the plain sum
    ("lrelu", 0, True, False, False, FINISH_SLOPE),
    ("pool", 0, False, False, True, FINISH_SLOPE),
    ("lrelu+pool", 0, True, False, True, FINISH_SLOPE),
    ("add1", 1, False, False, False, FINISH_SLOPE),
    ("add2+lrelu", 2, True, False, False, FINISH_SLOPE),
    ("add2+lrelu+pool", 2, True, False, True, FINISH_SLOPE),
    ("mask1", 1, False, True, False, FINISH_SLOPE),
    ("mask2", 2, False, True, False, FINISH_SLOPE),
    ("lrelu-0.1", 0, True, False, False, 0.1),               # not exact: held to bar(fp32 formula vs float64)
)


def exact_f32(x64):
    """The float64 result cast down, after asserting that fp32 holds it exactly (the comparison is then a bit comparison)."""
    x32 = x64.float()
    assert bool((x32.double() == x64).all()), "the reference left the exact regime"
    return x32


def avgpool_case(C, H, W, B=2):
    return int_tensor((B, C, H, W), torch.Generator().manual_seed(C * 1000 + H * 10 + W))


def upsample_case(Ca, Cb, h, w, B=2, bcast=False):
    """(a, b or None, cat): b has one batch entry when bcast (every entry of the batch reads it)."""
    g = torch.Generator().manual_seed(Ca * 100 + Cb * 10 + h + w)
    a = int_tensor((B, Ca, h, w), g)
    b = int_tensor((1 if bcast else B, Cb, h, w), g) if Cb else None
    return a, b, (a if b is None else torch.cat([a, b.expand(B, -1, -1, -1)], 1))


def finish_case(KS, C, H, W, B=2):
    """Integer-valued partial planes [KS * B, C, H, W] and the addends / mask sources for add_div 1 and 2."""
    g = torch.Generator().manual_seed(KS * 1000 + C * 10 + H + W)
    return {"part": int_tensor((KS * B, C, H, W), g), 1: int_tensor((B, C, H, W), g), 2: int_tensor((B // 2, C, H, W), g)}


def splitk_finish_ref(part, KS, add=None, add_div=1, slope=FINISH_SLOPE, lrelu=False, mask=False, pool=False, dtype=torch.float64):
    """The contract of ssm_splitk_finish_fwd (include/ssm_hip.h): y = act(sum_ks part[ks * B + b] + add[b / add_div]), the partial maps
    added in the order ks = 0, 1, ...; SSM_FLAG_MASK: y = sum * (add > 0 ? 1 : slope), no activation; pool = the 2x2 mean of y.
    Returns (y, pool or None)."""
    part = part.to(dtype)
    B = part.shape[0] // KS
    z = part[0:B].clone()
    for k in range(1, KS):
        z = z + part[k * B:(k + 1) * B]
    sl = torch.tensor(slope, dtype=dtype)          # slope 0.1: fp32(0.1) in the fp32 formula, 0.1 in float64
    if add is not None:
        a = add.to(dtype).repeat_interleave(add_div, 0)
        z = z * torch.where(a > 0, torch.ones_like(a), sl) if mask else z + a
    if lrelu:
        z = torch.maximum(z, z * sl)
    return z, (O.avg_pool2(z) if pool else None)
