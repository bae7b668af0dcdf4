"""fp64 and rounding-emulating restatements of the VGG19 perceptual loss (ir2rgb_amd/vgg.py) -- TEST INFRASTRUCTURE ONLY.

Four things, shared by tests/test_vgg_refs_cpu.py (no GPU), tests/test_vgg_fp64_gpu.py and tests/test_vgg_gpu.py:

* ``features64`` / ``loss64``: the feature chain and ``VGGLoss`` in fp64 on the operands the device path uses (the half
  copy of every weight, the half-rounded image, fp32 biases).
* ``emulated``: the same graph in fp32 torch with the device's rounding points, from oracle/emulated.py: ``rste``
  weights, ``rfb`` on the image and after each conv + bias + ReLU, torch max-pool, ``l1_half`` per term.  It records
  itself in the format of ``Recorder`` below, and ``fault=`` plants one named fault (FAULTS).
* one-stage references (``stage_fwd_ref``, ``stage_bwd_ref``, ``first_bwd_ref``): fp64 results of ONE convolution on
  the operands a run recorded, with the same operation on absolute values (S of oracle/bounds.py).
* the checks (``check_*``, ``run_checks``): what the GPU tests assert, as functions of a recording, so the CPU test can
  show that each rejects the planted faults and accepts the unfaulted emulation.

A recording (``Recorder``) holds, per convolution in call order (13 of the differentiated image, then 13 of the target):
the stage input ``x``, the stage output ``z``, the total gradient arriving at the output ``gz`` and the gradient the
stage sends to its input ``gx`` (None where no gradient flows); and for the loss assembly the features ``a`` / ``b``,
the value, and the gradient handed to each feature ``ga`` / ``gb``.

Inputs (tests' own, fixed here): weight ~ N(0, 2 / (9 Cin)), bias ~ N(0, 0.1^2) under a seeded generator -- every term
then holds a real share of the loss and the features stay O(1) -- and images tanh(randn), x and y independent.
"""
import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import bounds as B
from oracle import emulated as E
from oracle.replay import np64
from oracle.replay_ops import loss_chain

WEIGHTS = (1.0 / 32, 1.0 / 16, 1.0 / 8, 1.0 / 4, 1.0)          # models/loss.py:48 of the reference
SHAPES = ((2, 3, 35, 53), (1, 3, 17, 19))
FORMATS = {"bf16": torch.bfloat16, "f16": torch.float16}
GOUT = {"bf16": 1.0, "f16": 4096.0}                             # root of the backward pass (divided out afterwards: exact)
POOL_BEFORE = (2, 4, 8, 12)                                     # convolutions (in call order) that read a pooled tensor
SLICE_END = (0, 2, 4, 8, 12)                                    # convolutions whose output is relu{1..5}_1
LOSS_C_TERM = 4                                                 # roundings per summand of a loss slot (replay_loss_fwd)
DRIFT_FACTOR = 1.5

# name -> what is planted (``emulated(..., fault=name)``)
FAULTS = {
    "no_bias_conv4_1": "no bias in conv4_1",
    "leaky_conv3_2": "LeakyReLU(0.01) instead of ReLU in conv3_2",
    "no_mask_conv3_3": "no ReLU mask in conv3_3's backward",
    "avg_pool3": "average pool instead of the third max pool",
    "w1_x2": "term weight x2 on relu1_1",
    "w3_x1.25": "term weight x1.25 on relu3_1",
    "drop5": "relu5_1 term dropped",
    "wrong_n": "the L1 gradient of relu2_1 divides by relu1_1's element count",
}
_FAULT_CONV = {"no_bias_conv4_1": 8, "leaky_conv3_2": 5, "no_mask_conv3_3": 6}


# ---------------------------------------------------------------------------------------------------------------------
# inputs
def convs(vgg):
    """The 13 convolutions in call order."""
    return [m for s in range(1, 6) for m in getattr(vgg, f"slice{s}") if isinstance(m, nn.Conv2d)]


def init_weights(vgg, seed=11):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in convs(vgg):
            m.weight.copy_(torch.randn(m.weight.shape, generator=g) * math.sqrt(2.0 / (9 * m.in_channels)))
            m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
    return vgg


def images(shape, seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.tanh(torch.randn(shape, generator=g)), torch.tanh(torch.randn(shape, generator=g))


# ---------------------------------------------------------------------------------------------------------------------
# recording
class _Tap(torch.autograd.Function):
    """Identity whose backward notes the gradient that passes (rounded to ``dt`` first, where given)."""

    @staticmethod
    def forward(ctx, x, sink, key, dt):
        ctx.sink, ctx.key, ctx.dt = sink, key, dt
        # (not view_as: with a size-1 dimension it renumbers the strides, and fused_losses compares a's with b's)
        return x.as_strided(x.size(), x.stride())

    @staticmethod
    def backward(ctx, g):
        ctx.sink[ctx.key] = (g if ctx.dt is None else g.to(ctx.dt)).detach().clone()
        return g, None, None, None


def tap(x, sink, key, dt=None):
    return _Tap.apply(x, sink, key, dt)


def _hook(t, sink, key):
    t.register_hook(lambda g: sink.__setitem__(key, g.detach().clone()))


class Recorder:
    """Wrappers for ``ir2rgb_amd.vgg.A.conv_stage`` and ``ir2rgb_amd.vgg.fused_losses`` that record what passes."""

    def __init__(self):
        self.stages, self.loss = [], None

    def conv_stage(self, real):
        def wrapped(x, conv, *a, **kw):
            st = {"conv": conv, "x": x.detach(), "gz": None, "gx": None}
            if torch.is_grad_enabled() and x.requires_grad:
                x = tap(x, st, "gx")
            z = real(x, conv, *a, **kw)
            st["z"] = z.detach()
            if z.requires_grad:
                _hook(z, st, "gz")
            self.stages.append(st)
            return z
        return wrapped

    def fused_losses(self, real):
        def wrapped(terms, nslots, dtype):
            ls = {"a": [t[1].detach() for t in terms], "b": [t[2].detach() for t in terms], "w": [t[3] for t in terms],
                  "ga": [None] * len(terms), "gb": [None] * len(terms)}
            bs = [t[2].detach().requires_grad_() for t in terms]          # leaves: any gradient handed to them shows
            ls["b_leaves"] = bs
            new = [(t[0], tap(t[1], ls["ga"], i) if t[1].requires_grad else t[1], bs[i]) + tuple(t[3:])
                   for i, t in enumerate(terms)]
            out = real(new, nslots, dtype)
            ls["value"] = out.detach()[0]
            self.loss = ls
            return out
        return wrapped

    def finish(self):
        """After the backward pass: the gradients the loss handed to the target's features (None: nothing)."""
        if self.loss is not None and "b_leaves" in self.loss:
            self.loss["gb"] = [t.grad for t in self.loss.pop("b_leaves")]
        return self


def to_cpu(rec):
    """A device recording as CPU fp32 NCHW-contiguous tensors (values unchanged: half -> fp32 is exact)."""
    def c(t):
        return None if t is None else t.detach().float().cpu().contiguous()
    out = Recorder()
    out.stages = [dict(st, x=c(st["x"]), z=c(st["z"]), gz=c(st["gz"]), gx=c(st["gx"])) for st in rec.stages]
    if rec.loss is not None:
        ls = rec.loss
        out.loss = dict(ls, a=[c(t) for t in ls["a"]], b=[c(t) for t in ls["b"]], ga=[c(t) for t in ls["ga"]],
                        gb=[c(t) for t in ls["gb"]], value=float(ls["value"].double().item()))
    return out


def device_record(loss_mod, x, y, fmt):
    """``loss_mod(x, y)`` (an ir2rgb_amd.vgg.VGGLoss on the GPU) forward and backward, rooted at GOUT[fmt], with every
    convolution stage and the loss assembly recorded -> (Recorder of CPU tensors, d loss / d x on the CPU).  ``x`` must
    be a leaf that requires grad."""
    import ir2rgb_amd.vgg as V
    rec = Recorder()
    real_cs, real_fl = V.A.conv_stage, V.fused_losses
    V.A.conv_stage, V.fused_losses = rec.conv_stage(real_cs), rec.fused_losses(real_fl)
    try:
        loss = loss_mod(x, y)
        loss.backward(torch.full_like(loss, GOUT[fmt]))
    finally:
        V.A.conv_stage, V.fused_losses = real_cs, real_fl
    torch.cuda.synchronize()
    rec.finish()
    return to_cpu(rec), (x.grad.detach().double() / GOUT[fmt]).cpu()


# ---------------------------------------------------------------------------------------------------------------------
# fp64 chain
def features64(vgg, img, dt):
    """relu{1..5}_1 in fp64 from ``img`` (fp64, already rounded to ``dt`` by the caller) and the half weights."""
    h, outs = img, []
    for s in range(1, 6):
        for m in getattr(vgg, f"slice{s}"):
            if isinstance(m, nn.Conv2d):
                h = F.relu(F.conv2d(h, m.weight.detach().to(dt).double(), m.bias.detach().double(), 1, 1))
            elif isinstance(m, nn.MaxPool2d):
                h = F.max_pool2d(h, 2, 2)
        outs.append(h)
    return outs


def loss64(fx, fy):
    return sum(w * (a - b.detach()).abs().mean() for a, b, w in zip(fx, fy, WEIGHTS))


def reference64(vgg, x, y, dt):
    """-> {"fx", "fy" (detached fp64 features), "loss" (float), "grad" (d loss / d x, fp64)} on the rounded operands."""
    x64 = x.to(dt).double().requires_grad_()
    fx = features64(vgg, x64, dt)
    with torch.no_grad():
        fy = features64(vgg, y.to(dt).double(), dt)
    loss = loss64(fx, fy)
    grad, = torch.autograd.grad(loss, x64)
    return {"fx": [t.detach() for t in fx], "fy": fy, "loss": float(loss.item()), "grad": grad,
            "terms": [float(w * (a.detach() - b).abs().mean()) for a, b, w in zip(fx, fy, WEIGHTS)]}


# ---------------------------------------------------------------------------------------------------------------------
# rounding-emulating chain
class _ReluNoMask(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return F.relu(x)

    @staticmethod
    def backward(ctx, g):
        return g


class _L1WrongN(torch.autograd.Function):
    """emulated.l1_half with the gradient divided by another term's element count (fault 'wrong_n')."""

    @staticmethod
    def forward(ctx, a, b, weight, dt, n):
        ctx.save_for_backward(a, b)
        ctx.weight, ctx.dt, ctx.n = weight, dt, n
        return (a - b).abs().mean() * weight

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        s = g.float() * (torch.tensor(ctx.weight, dtype=torch.float32) / torch.tensor(float(ctx.n), dtype=torch.float32))
        return torch.sign(a - b) * s.to(ctx.dt).float(), None, None, None, None


def emulated_features(vgg, img, dt, rec, fault=None, perm_seed=None):
    """The feature chain with the device's rounding points (fp32 CPU tensors holding half values); appends the 13 stages
    to ``rec``.  ``perm_seed``: permute the input channels of every convolution (another summation order)."""
    g = None if perm_seed is None else torch.Generator().manual_seed(perm_seed)
    h, outs, k = E.rfb(img, dt), [], 0
    for s in range(1, 6):
        for m in getattr(vgg, f"slice{s}"):
            if isinstance(m, nn.Conv2d):
                st = {"conv": m, "x": h.detach(), "gz": None, "gx": None}
                xin = tap(h, st, "gx", dt if k else None) if h.requires_grad else h
                w = E.rste(m.weight.detach(), dt)
                if g is not None:
                    p = torch.randperm(m.in_channels, generator=g)
                    pre = F.conv2d(xin[:, p].contiguous(), w[:, p].contiguous(), None, 1, 1)
                else:
                    pre = F.conv2d(xin, w, None, 1, 1)
                if not (fault == "no_bias_conv4_1" and k == _FAULT_CONV[fault]):
                    pre = pre + m.bias.detach().view(1, -1, 1, 1)
                if fault == "leaky_conv3_2" and k == _FAULT_CONV[fault]:
                    r = F.leaky_relu(pre, 0.01)
                elif fault == "no_mask_conv3_3" and k == _FAULT_CONV[fault]:
                    r = _ReluNoMask.apply(pre)
                else:
                    r = F.relu(pre)
                if r.requires_grad:
                    _hook(r, st, "gz")          # (behind rfb's backward: the total gradient as the half tensor holds it)
                h = E.rfb(r, dt)
                st["z"] = h.detach()
                rec.stages.append(st)
                k += 1
            elif isinstance(m, nn.MaxPool2d):
                h = F.avg_pool2d(h, 2, 2) if fault == "avg_pool3" and k == 8 else F.max_pool2d(h, 2, 2)
        outs.append(h)
    return outs


def emulated(vgg, x, y, fmt, fault=None, perm_seed=None):
    """Forward and backward of the emulated loss -> (Recorder of CPU tensors, d loss / d x as fp32)."""
    dt = FORMATS[fmt]
    rec = Recorder()
    x = x.clone().requires_grad_()
    fx = emulated_features(vgg, x, dt, rec, fault, perm_seed)
    with torch.no_grad():
        fy = emulated_features(vgg, y, dt, rec, fault, perm_seed)
    ws = list(WEIGHTS)
    if fault == "w1_x2":
        ws[0] *= 2
    if fault == "w3_x1.25":
        ws[2] *= 1.25
    ls = {"a": [t.detach() for t in fx], "b": [t.detach() for t in fy], "w": ws, "ga": [None] * 5, "gb": [None] * 5}
    total = 0.0
    for i, (a, b, w) in enumerate(zip(fx, fy, ws)):
        if fault == "drop5" and i == 4:
            continue
        a = tap(a, ls["ga"], i)
        if fault == "wrong_n" and i == 1:
            total = total + _L1WrongN.apply(a, b.detach(), float(w), dt, fx[0].numel())
        else:
            total = total + E.l1_half(a, b, w, dt)
    ls["value"] = float(total.detach().double().item())
    rec.loss = ls
    (total * GOUT[fmt]).backward()
    return rec, x.grad / GOUT[fmt]


# ---------------------------------------------------------------------------------------------------------------------
# one-stage fp64 references
def _w64(conv, dt):
    return conv.weight.detach().cpu().to(dt).double(), conv.bias.detach().cpu().double()


def stage_fwd_ref(x, conv, dt):
    """(pre-activation, S) of one convolution on the recorded input ``x`` (rounded to ``dt``: a no-op but for the image)."""
    w, b = _w64(conv, dt)
    x64 = x.to(dt).double()
    return F.conv2d(x64, w, b, 1, 1), F.conv2d(x64.abs(), w.abs(), b.abs(), 1, 1)


def stage_bwd_ref(gz, z, conv, dt):
    """(input gradient of gz * [z > 0], S): the mask from the recorded output, the product exact in half."""
    w, _ = _w64(conv, dt)
    gy = gz.double() * (z > 0)
    return F.conv_transpose2d(gy, w, None, 1, 1), F.conv_transpose2d(gy.abs(), w.abs(), None, 1, 1)


def _shift(t, kx):
    """Column ox of the x-im2col tap kx is image column ox + kx - 1 (zero padding 1): partials -> image columns."""
    W = t.shape[-1]
    out = torch.zeros_like(t)
    lo, hi = max(0, 1 - kx), min(W, W + 1 - kx)
    out[..., lo + kx - 1:hi + kx - 1] = t[..., lo:hi]
    return out


def first_bwd_ref(gz, z, conv, fmt):
    """(fp32 image gradient reference, its bound) of the first layer.

    The device writes it in two steps (autograd._image_grad).  Step 1 is the adjoint of the (3 x 1) convolution over the
    x-expanded image: for every tap kx a partial p_kx[c, y, ox] = sum over (co, ky) of gy[co, y - ky + 1, ox] *
    w[co, c, ky, kx], a chain of 3 * Cout products accumulated in fp32 and STORED IN HALF, so the stored value p'_kx is
    within e_kx = bounds.bound(p_kx, S_kx, fmt, 3 * Cout + 2) of p_kx.  Step 2 is the x-im2col adjoint in fp32:
    dx[c, y, x] = sum over the at most three kx with 0 <= x - kx + 1 < W of p'_kx[c, y, x - kx + 1], a three-term fp32
    sum, within bounds.bound_sum(., sum |p'_kx|, "f32", 3) of the exact sum of the p'.  Composed, with |p'| <= |p| + e:

        |dx - ref| <= sum_kx e_kx + gamma_3 * sum_kx (|p_kx| + e_kx) + eta_f32,      ref = sum_kx p_kx.
    """
    w, _ = _w64(conv, FORMATS[fmt])
    gy = gz.double() * (z > 0)
    ref = esum = ssum = 0.0
    for kx in range(3):
        wk = w[:, :, :, kx:kx + 1].contiguous()
        p = F.conv_transpose2d(gy, wk, None, 1, (1, 0))
        Sp = F.conv_transpose2d(gy.abs(), wk.abs(), None, 1, (1, 0))
        e = torch.from_numpy(B.bound(np64(p), np64(Sp), fmt, 3 * conv.out_channels + 2))
        ref = ref + _shift(p, kx)
        esum = esum + _shift(e, kx)
        ssum = ssum + _shift(p.abs() + e, kx)
    bnd = np64(esum) + B.bound_sum(np64(ref), np64(ssum), "f32", 3)
    return np64(ref), bnd


# ---------------------------------------------------------------------------------------------------------------------
# checks.  Each returns a ratio: <= 1 passes, > 1 (inf for a bit-for-bit check with mismatches) rejects.
def _worst(got, ref, bnd):
    ok, ratio, _, _ = B.check_bound(np64(got), ref, bnd)
    return ratio


def check_stage_fwd(st, fmt):
    """|z - relu(ref_pre)| <= bounds.bound(ref_pre, S, fmt, 9 Cin + 2), every element."""
    conv = st["conv"]
    pre, S = stage_fwd_ref(st["x"], conv, FORMATS[fmt])
    pre, S = np64(pre), np64(S)
    chain = B.chain_fwd({"kh": 3, "kw": 3, "Cin": conv.in_channels})
    return _worst(st["z"], np.maximum(pre, 0.0), B.bound(pre, S, fmt, chain))


def check_stage_bwd(st, fmt, first):
    """|g_in - ref| <= bounds.bound(ref, S, fmt, 9 Cout + 2); the first layer under first_bwd_ref's composed bound."""
    conv = st["conv"]
    if st["gx"] is None or st["gz"] is None:
        return math.inf
    if first:
        ref, bnd = first_bwd_ref(st["gz"], st["z"], conv, fmt)
        return _worst(st["gx"], ref, bnd)
    ref, S = stage_bwd_ref(st["gz"], st["z"], conv, FORMATS[fmt])
    ref, S = np64(ref), np64(S)
    return _worst(st["gx"], ref, B.bound(ref, S, fmt, 9 * conv.out_channels + 2))


def check_pools(stages):
    """Stage inputs are the previous output (max-pooled where the graph pools), bit for bit: -> mismatching elements."""
    bad = 0
    for k in range(1, len(stages)):
        if k % 13 == 0:
            continue
        prev = stages[k - 1]["z"]
        want = F.max_pool2d(prev, 2, 2) if k % 13 in POOL_BEFORE else prev
        x = stages[k]["x"]
        bad += int((x != want).sum()) if x.shape == want.shape else x.numel()
    return bad


def loss_reference(a, b):
    """fp64 value and S of sum_i w_i mean|a_i - b_i|, and the bound of the fp32 loss slot."""
    items = [{"n": t.numel(), "kind": 0} for t in a]
    ref = sum(w * np.abs(np64(x) - np64(y)).mean() for x, y, w in zip(a, b, WEIGHTS))
    S = sum(w * (np.abs(np64(x)) + np.abs(np64(y))).mean() for x, y, w in zip(a, b, WEIGHTS))
    chain = max(loss_chain({"items": items}, i) for i in range(len(items)))
    return float(ref), float(B.bound_rw(np.float64(ref), np.float64(S), "f32", chain, LOSS_C_TERM))


def check_loss_value(ls):
    ref, bnd = loss_reference(ls["a"], ls["b"])
    v = ls["value"]
    return abs(v - ref) / bnd if math.isfinite(v) else math.inf


def check_loss_grads(ls, fmt):
    """Every feature of x gets sign(a_i - b_i) * half(gout * (w_i / n_i)) bit for bit (the fp32 product the kernel forms),
    the features of y nothing: -> mismatching elements."""
    dt = FORMATS[fmt]
    bad = 0
    for a, b, w, ga, gb in zip(ls["a"], ls["b"], WEIGHTS, ls["ga"], ls["gb"]):
        if gb is not None:
            bad += gb.numel()
        if ga is None:
            bad += a.numel()
            continue
        s = torch.tensor(GOUT[fmt], dtype=torch.float32) * (torch.tensor(w, dtype=torch.float32)
                                                            / torch.tensor(float(a.numel()), dtype=torch.float32))
        want = torch.sign(a.double() - b.double()) * s.to(dt).double()
        bad += int((ga.double() != want).sum())
    return bad


def end_to_end(ls, ref):
    """Both sides of |loss - loss_fp64| <= sum_i w_i (mean|a'_i - a_i| + mean|b'_i - b_i|) + (the loss slot's bound):
    the triangle inequality through the fp64 loss of the recorded features a', b'."""
    _, bnd = loss_reference(ls["a"], ls["b"])
    rhs = sum(w * (np.abs(np64(a1) - np64(a)).mean() + np.abs(np64(b1) - np64(b)).mean())
              for a1, b1, a, b, w in zip(ls["a"], ls["b"], ref["fx"], ref["fy"], WEIGHTS)) + bnd
    return abs(ls["value"] - ref["loss"]), float(rhs)


def rel_l2(got, ref):
    got, ref = np64(got), np64(ref)
    return float(np.linalg.norm(got - ref) / np.linalg.norm(ref))


def drift(feats, grad, ref):
    """Per-slice relative L2 of the features of x against the fp64 chain, and of the image gradient."""
    return [rel_l2(a1, a) for a1, a in zip(feats, ref["fx"])], rel_l2(grad, ref["grad"])


NOISE_DRAWS = 8


def noise_level(vgg, x, y, fmt, ref):
    """The calibration of the drift checks: drift() of the emulation against the fp64 chain, as the root mean square
    over NOISE_DRAWS evaluations that round at the same places in different summation orders (the plain one and
    channel permutations 1 .. NOISE_DRAWS - 1).  One draw is a noisy estimate of the level where few elements carry the
    norm: the image gradient at 17 x 19 has 969 elements and moves with single L1 sign flips, and its draws spread by
    +-15 % (f16: 0.040 .. 0.057 over CPUs and orders); the mean square over draws estimates the same level with a third
    of that spread.  Nothing of the code under test enters."""
    sq_f, sq_g = np.zeros(5), 0.0
    for k in range(NOISE_DRAWS):
        rec, grad = emulated(vgg, x, y, fmt, perm_seed=k or None)
        f, g = drift(rec.loss["a"], grad, ref)
        sq_f, sq_g = sq_f + np.square(f), sq_g + g * g
    return [float(v) for v in np.sqrt(sq_f / NOISE_DRAWS)], math.sqrt(sq_g / NOISE_DRAWS)


def run_checks(rec, grad, ref, noise, fmt):
    """Every check of tests/test_vgg_fp64_gpu.py on one recording -> {name: ratio} (> 1 rejects) and the per-stage
    ratios.  ``noise``: drift() of the unfaulted emulation (the calibration of the two drift checks)."""
    fwd = [check_stage_fwd(st, fmt) for st in rec.stages]
    bwd = [check_stage_bwd(st, fmt, k == 0) for k, st in enumerate(rec.stages[:13])]
    lhs, rhs = end_to_end(rec.loss, ref)
    dfeat, dgrad = drift(rec.loss["a"], grad, ref)
    out = {"stage_fwd": max(fwd), "stage_bwd": max(bwd),
           "pools": math.inf if check_pools(rec.stages) else 0.0,
           "loss_value": check_loss_value(rec.loss),
           "loss_grads": math.inf if check_loss_grads(rec.loss, fmt) else 0.0,
           "end_to_end": lhs / rhs,
           "drift_features": max(d / (DRIFT_FACTOR * n) for d, n in zip(dfeat, noise[0])),
           "drift_gradient": dgrad / (DRIFT_FACTOR * noise[1])}
    return out, {"fwd": fwd, "bwd": bwd, "drift_features": dfeat, "drift_gradient": dgrad, "end_to_end": (lhs, rhs)}
