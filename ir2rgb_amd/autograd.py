"""torch.autograd bindings of the fused HIP stages (what ``loss.backward()`` walks).

Each stage of ir2rgb_amd.layers gets a ``torch.autograd.Function`` whose backward is again a
short sequence of libir2rgb_hip.so calls:

    gz --bn_bwd--> gy (grad wrt conv output), dgamma, dbeta
    gy --conv2d_fwd with the adjoint geometry (+ fold_reflect / xexpand_bwd)--> dx
    (x, gy) --wgrad--> dW

Status of the pieces (see DESIGN.md "what is hand-written"): activation/BatchNorm backward, all
data gradients, weight gradients (MFMA, transposed LDS reads), reflection fold and x-im2col adjoint
are HIP, as are the backward of the separable head convolutions and of the warp-blend.  No torch
convolution is left on the generator / discriminator path, forward or backward.
"""
import contextlib
import os

import torch
import torch.nn.functional as F
from torch.autograd import Function

from . import _lib
from . import conv as C
from . import layers as L
from . import stageplan
from . import streamcheck as SC

_DT = C._TORCH2DT
_ADJ_DESCS = {}      # adjoint descriptors of strided convolutions (dgrad_geometry), one object per geometry


def _as_half_nhwc(g, dtype):
    if g.dtype == dtype and C.is_nhwc(g):
        return g
    if g.dtype == torch.float32:
        return L.to_nhwc_half(g, dtype)
    return g.to(dtype).contiguous(memory_format=torch.channels_last)


BN_BWD_FROZEN, BN_BWD_ACCUMULATE = 16, 32      # IR2RGB_BN_BWD_FROZEN / _ACCUMULATE of include/ir2rgb_hip.h, or-ed into act


def bn_bwd(gz, y, scale, shift, mean, invstd, act, out=None, params=None):
    """-> (gy, dgamma, dbeta).  scale None: activation-only stage (dbeta is then the bias gradient).  ``out``: where gy
    goes (a sample-group slice of the batch's gradient tensor, see ConvStageFn); ``params`` = (dgamma, dbeta) of an earlier
    group of the same layer: this group's are added to them in the kernel (act | BN_BWD_ACCUMULATE)."""
    n, ch, h, w = y.shape
    npix = n * h * w
    nblk = _lib.query("ir2rgb_bn_bwd_blocks", npix, ch)
    dev = y.device
    if params is not None:
        dgamma, dbeta = params
        act |= BN_BWD_ACCUMULATE
        buf = torch.empty((nblk * 2 + 3) * ch, dtype=torch.float32, device=dev)
        ppartial = buf.data_ptr()
    else:
        # one allocation: [dgamma | dbeta | the kernel's partial rows] (the rows only ever exist as an address)
        buf = torch.empty((nblk * 2 + 5) * ch, dtype=torch.float32, device=dev)
        dgamma, dbeta = buf[:ch], buf[ch:2 * ch]
        ppartial = buf.data_ptr() + 8 * ch
    gy = out if out is not None else torch.empty_like(y, memory_format=torch.channels_last)
    _lib.launch("ir2rgb_bn_bwd", y, gz, y, scale, shift, mean, invstd, gy, dgamma, dbeta, ppartial, npix, ch, act, _DT[y.dtype])
    return gy, dgamma, dbeta


def thin_grad_expand(gz, dtype):
    """fp32 gradient [N,Cout<=8,H,W] of a thin output -> (g64, g8, dbias): 64- and 8-channel zero-padded
    channels_last half copies and the per-channel sum, one launch."""
    gz = gz.float().contiguous()
    n, cout, h, w = gz.shape
    g64 = C.empty_nhwc(n, 64, h, w, dtype, gz.device)
    g8 = C.empty_nhwc(n, 8, h, w, dtype, gz.device)
    dbias = torch.empty(cout, dtype=torch.float32, device=gz.device)
    _lib.launch("ir2rgb_thin_grad_expand", gz, gz, g64, g8, dbias, n, cout, h, w, _DT[dtype])
    return g64, g8, dbias


def fold_reflect(dxpad, pad_h, pad_w=None):
    pad_w = pad_h if pad_w is None else pad_w
    n, ch, hp, wp = dxpad.shape
    h, w = hp - 2 * pad_h, wp - 2 * pad_w
    dx = C.empty_nhwc(n, ch, h, w, dxpad.dtype, dxpad.device)
    _lib.launch("ir2rgb_fold_reflect", dxpad, dxpad, dx, n, h, w, ch, pad_h, pad_w, _DT[dxpad.dtype])
    return dx


def xexpand_bwd(dxe, cin, w, kw, stride_w, pad_w, pad_mode):
    n, _, h, wout = dxe.shape
    din = torch.empty((n, cin, h, w), dtype=torch.float32, device=dxe.device)
    _lib.launch("ir2rgb_xexpand_bwd", dxe, dxe, din, n, cin, h, w, wout, kw, stride_w, pad_w, pad_mode, _DT[dxe.dtype])
    return din


# ---------------------------------------------------------------------------------------------
# data gradient = a forward convolution with the adjoint geometry
# ---------------------------------------------------------------------------------------------
def _compose(f, g):
    if f is None:
        return g
    if g is None:
        return f
    return lambda w: g(f(w))


# ---------------------------------------------------------------------------------------------
# channel padding: any ngf / ndf behind the reference's factories (networks.py:51-82; generator.py:36 halves ngf per
# spatial scale).  The MFMA kernels want 64-multiples (BatchNorm backward: powers of two), so a layer whose width is not
# one runs at the next power of two >= 64: zero weight rows / columns, zero BatchNorm shift for the extra channels, which
# therefore stay exactly zero through convolution, BatchNorm (0 * scale + 0), ReLU and residual adds, forward and backward.
# Parameters and their gradients keep the reference's shapes.  Widths that are 64-multiples take none of this.
# ---------------------------------------------------------------------------------------------
def padded_width(c):
    return c if c % 64 == 0 and (c & (c - 1)) == 0 else max(64, 1 << (c - 1).bit_length())


def _pad_weight_fn(cout_to, cin_to, transposed):
    """Conv2d weight [Cout,Cin,kh,kw] (ConvTranspose2d: [Cin,Cout,kh,kw]) -> zero-padded to the widths the kernels run at."""
    def f(w):
        a, b = (cin_to, cout_to) if transposed else (cout_to, cin_to)
        return L.pad_dim(L.pad_dim(w, 0, a), 1, b)
    return f


class PadChannelsFn(Function):
    """[N,C,H,W] half -> [N,Cp,H,W] channels_last half with zero extra channels (a tensor entering the padded domain from
    outside: coarse features, a stand-alone ResnetBlock call); the gradient is the slice."""

    @staticmethod
    def forward(ctx, x, cp):
        ctx.c = x.shape[1]
        out = torch.zeros((x.shape[0], cp, x.shape[2], x.shape[3]), dtype=x.dtype, device=x.device).contiguous(
            memory_format=torch.channels_last)
        out[:, :ctx.c] = x
        return out

    @staticmethod
    def backward(ctx, g):
        return g[:, :ctx.c], None


def pad_channels(x, cp):
    return x if x.shape[1] == cp else PadChannelsFn.apply(x, cp)


class _PaddedBN:
    """nn.BatchNorm2d seen at a padded width by bn_finalize: gamma 1 / beta 0 / running (0, 1) for the extra channels;
    ``commit`` writes the real channels' running statistics back."""

    def __init__(self, bn, cp):
        self.bn, self.num_features = bn, cp
        self.weight = L.pad_dim(bn.weight.detach(), 0, cp, 1.0)
        self.bias = L.pad_dim(bn.bias.detach(), 0, cp, 0.0)
        self.track_running_stats, self.momentum, self.eps = bn.track_running_stats, bn.momentum, bn.eps
        self.running_mean = None if bn.running_mean is None else L.pad_dim(bn.running_mean, 0, cp, 0.0)
        self.running_var = None if bn.running_var is None else L.pad_dim(bn.running_var, 0, cp, 1.0)
        self.num_batches_tracked = bn.num_batches_tracked

    def commit(self, training):
        if training and self.track_running_stats and self.running_mean is not None:
            c = self.bn.num_features
            self.bn.running_mean.copy_(self.running_mean[:c])
            self.bn.running_var.copy_(self.running_var[:c])


def dgrad_geometry(spec, x_shape, gy_shape, dtype):
    """The data gradient of the convolution ``spec`` over an input of ``x_shape`` as a forward launch on the gradient
    ``gy_shape`` w.r.t. its output: -> (launch descriptor, descriptor the weight is packed for, adjoint packing, fold).
    ``fold``: the launch writes the gradient of the reflection-PADDED input and fold_reflect follows."""
    kh, kw = spec["k"]
    (sh, sw), (ph, pw) = spec["stride"], spec["pad"]
    n, cin, hin, win = x_shape
    if spec["transposed"]:
        # forward was ConvTranspose2d(W[cin][cout]); adjoint = Conv2d with the same memory as [out=cin][in=cout]
        desc = C.make_desc(gy_shape, cin, (kh, kw), (sh, sw), (ph, pw), C.PAD_ZERO, dtype)
        return desc, desc, False, False
    if sh == 1 and sw == 1:
        if spec["pad_mode"] != C.PAD_REFLECT:
            desc = C.make_desc(gy_shape, cin, (kh, kw), 1, (kh - 1 - ph, kw - 1 - pw), C.PAD_ZERO, dtype)
            return desc, desc, True, False
        if (kh, kw, ph, pw) == (3, 3, 1, 1):
            # the patch-staged kernel evaluates the adjoint of the reflection in place (border terms):
            # no padded 2-pixel-larger output grid, no fold pass
            dadj = C.make_desc(gy_shape, cin, 3, 1, 1, C.PAD_REFLECT_ADJ, dtype)
            if C.kernel_name(dadj) == "conv3x3_patch_kernel":
                return dadj, C.make_desc(gy_shape, cin, 3, 1, 1, C.PAD_ZERO, dtype), True, False
        desc = C.make_desc(gy_shape, cin, (kh, kw), 1, (kh - 1, kw - 1), C.PAD_ZERO, dtype)
        return desc, desc, True, True
    # strided zero-padded convolution: adjoint = transposed convolution reading W as [in=cout][out=cin]
    if spec["pad_mode"] != C.PAD_ZERO:
        raise NotImplementedError("data gradient of a strided reflect-padded convolution")
    hfull, wfull = (gy_shape[2] - 1) * sh - 2 * ph + kh, (gy_shape[3] - 1) * sw - 2 * pw + kw
    assert 0 <= hin - hfull < sh and 0 <= win - wfull < sw, "adjoint geometry mismatch"
    key = (n, gy_shape[2], gy_shape[3], gy_shape[1], hin, win, cin, kh, kw, sh, sw, ph, pw, C.PAD_ZERO, 1, _DT[dtype], 0, 0, 0, 0, 0, 0)
    desc = _ADJ_DESCS.get(key)
    if desc is None:
        desc = _ADJ_DESCS[key] = C.sealed(C.ConvDesc(*key))
    return desc, desc, False, False


def conv_dgrad(gy, conv, spec, x_shape, weight_fn=None, tag="dgrad", out=None):
    """gy: grad wrt the convolution output (channels_last half, channels % 64 == 0).  ``weight_fn``
    maps conv.weight to the weight tensor the forward convolution actually used (x-expanded / padded
    forms).  Returns grad wrt the convolution input (channels_last half)."""
    desc, dpack, adjoint, fold = dgrad_geometry(spec, x_shape, tuple(gy.shape), gy.dtype)
    wp = L.packed_weight(conv, dpack, weight_fn, tag=tag, adjoint=adjoint)
    if not fold:
        return C.conv2d_fwd(desc, gy, wp, out=out)[0]
    dxpad, _ = C.conv2d_fwd(desc, gy, wp)
    ph, pw = spec["pad"]
    dx = fold_reflect(dxpad, ph, pw) if (ph or pw) else dxpad
    return dx if out is None else out.copy_(dx)


# ---------------------------------------------------------------------------------------------
# weight gradient: MFMA kernel (wgrad_mfma.hip).  Thin gradients (the 1-channel PatchGAN logits)
# are zero-padded to 8 channels so they take the same kernel.
# ---------------------------------------------------------------------------------------------
# Gradient sinks (data-parallel runs): weight parameter -> its slice of the optimizer's flat all-reduce buffer.  A
# convolution whose weight is registered here writes its weight gradient straight into that slice and returns it, so
# autograd adopts a tensor that already lives in the buffer and no gather copy precedes the all-reduce.  Only sound for
# a parameter that receives ONE contribution per backward pass (the caller's promise: flatgrads.FlatGrads(direct=True)).
# SINK_STREAMS: weight parameter -> the stream its sink was last written on.  A backward node runs on the stream of its
# forward (the finer generators' branches: two streams), and whoever reads a range of the buffer from inside the pass --
# the hook that puts a chunk on the wire -- has to wait for each of them (flatgrads.FlatGrads._join_writers).
GRAD_SINKS = {}
SINK_STREAMS = {}


def wgrad_destination(weight, shape):
    """Where the gradient of ``weight`` (a layer running at the parameter's own ``shape``) is written and what autograd is
    handed for it: -> (out, accumulate, grad).  ``out`` None: a fresh tensor, which is then the gradient."""
    sink = GRAD_SINKS.get(weight) if GRAD_SINKS else None
    have = weight.grad
    if (sink is None and have is not None and have.dtype is torch.float32 and have.is_contiguous()
            and have.shape == weight.shape):
        # a later use of the same parameter in this pass (the discriminators see two or three inputs per window): dw is
        # added to .grad by the kernel's own finish pass; autograd gets nothing to add
        return have, True, None
    if sink is None:
        return None, False, None
    if tuple(sink.shape) != shape or sink.dtype is not torch.float32 or not sink.is_contiguous():
        raise ValueError("conv2d_wgrad: out must be a contiguous fp32 tensor of the weight's shape on the inputs' device")
    # (a NEW tensor object over the sink's memory: autograd adopts a gradient without cloning it only when nobody else
    # holds the object it is handed)
    SINK_STREAMS[weight] = torch.cuda.current_stream(sink.device)     # (the caller launches on the current stream)
    return sink, False, sink.view(shape)


def conv_wgrad(x, gy, weight_shape, spec, out=None, accumulate=False):
    cin, cout = x.shape[1], gy.shape[1]
    if cin % 8:
        raise NotImplementedError("weight gradient needs an input channel count that is a multiple of 8")
    if cout % 8:
        if spec["transposed"]:
            raise NotImplementedError("thin transposed convolutions do not occur on this path")
        pad = (-cout) % 8
        gp = torch.zeros((gy.shape[0], cout + pad, gy.shape[2], gy.shape[3]), dtype=gy.dtype, device=gy.device).contiguous(
            memory_format=torch.channels_last)
        gp[:, :cout] = gy
        desc = C.make_desc(tuple(x.shape), cout + pad, spec["k"], spec["stride"], spec["pad"], spec["pad_mode"], x.dtype)
        return C.conv2d_wgrad(desc, x, gp)[:cout].contiguous()
    desc = C.make_desc(tuple(x.shape), cout, spec["k"], spec["stride"], spec["pad"], spec["pad_mode"], x.dtype,
                       bool(spec["transposed"]), spec.get("output_padding", 0))
    return C.conv2d_wgrad(desc, x, gy, out=out, accumulate=accumulate)


# ---------------------------------------------------------------------------------------------
# weight gradients on a second HIP stream (OFF by default since the nine-tap weight-gradient kernel: see below).
# The data-gradient chain (dgrad conv -> BN backward of the layer below) is the critical path of
# loss.backward(); the weight gradient of a layer only feeds the optimizer, so it can run beside that chain
# and fill the CUs the chain's small launches leave idle.  This is only sound for a parameter that is used
# ONCE per backward pass: autograd then hands the tensor to AccumulateGrad untouched.  A parameter used by
# several nodes has its contributions summed by the engine on the main stream, which knows nothing of the
# side stream (measured: discriminator gradients, 3 uses per pass, came out wrong).  So the side stream is
# opt-in per module tree (enable_side_wgrad: the trainer marks the generators, each called once per window)
# and never used while the parameter already holds a gradient.  The side stream is joined when the backward
# pass ends (engine callback).
# Measured: with the one-tap weight-gradient kernel (126 us, half of the chip idle) the overlap saved 2 ms per
# window; with the nine-tap kernel (44 us, every CU busy) it COSTS 1.7 ms (44.2 vs 42.5 ms per window): the
# overlapped kernels slow the critical chain and the stream hand-offs add bubbles (sending only the remaining one-tap
# launches to the side stream measured no better: 44.3 ms).  Hence default off (IR2RGB_WGRAD_STREAM=1 enables it;
# tests/test_losses_gpu.py keeps it covered).
# ---------------------------------------------------------------------------------------------
WGRAD_SIDE_STREAM = os.environ.get("IR2RGB_WGRAD_STREAM", "0") != "0"
_SIDE_PENDING = set()       # devices whose side stream the running backward pass has used


def _join_side(dev, side):
    _SIDE_PENDING.discard(dev)
    C.SIDE_BUSY = False
    torch.cuda.current_stream(dev).wait_stream(side)


def enable_side_wgrad(module, enabled=True):
    """Allow (or forbid) side-stream weight gradients for every convolution under ``module``.  The caller
    asserts that each of these convolutions is applied once per backward pass."""
    for m in module.modules():
        if isinstance(m, (torch.nn.Conv2d, torch.nn.ConvTranspose2d)):
            m._ir2rgb_side_wgrad = bool(enabled)


def wgrad_overlapped(conv, fn, *inputs):
    """Run ``fn()`` (the weight-gradient computation of ``conv`` reading ``inputs``) on the side stream
    when that is safe (see above), else on the current stream."""
    dev = inputs[0].device
    param = conv.weight
    if not WGRAD_SIDE_STREAM or dev.type != "cuda" or not getattr(conv, "_ir2rgb_side_wgrad", False):
        return fn()
    if GRAD_SINKS and param in GRAD_SINKS:
        # the gradient goes straight into the all-reduce buffer, and the hook that puts its chunk on the wire waits for the
        # streams wgrad_destination saw (SINK_STREAMS: the node's own stream, main or the generators' branch stream), not
        # for SLOT_WGRAD: a sink is never written from there
        return fn()
    from .networks import SLOT_WGRAD, side_stream      # (networks imports this module)
    main, side = torch.cuda.current_stream(dev), side_stream(dev, SLOT_WGRAD)
    if param.grad is not None:
        main.wait_stream(side)
        return fn()
    side.wait_stream(main)
    with torch.cuda.stream(side):
        out = fn()
    for t in inputs:
        t.record_stream(side)
    out.record_stream(main)
    if dev not in _SIDE_PENDING:
        _SIDE_PENDING.add(dev)
        C.SIDE_BUSY = True
        torch.autograd.Variable._execution_engine.queue_callback(lambda: _join_side(dev, side))
    return out


# ---------------------------------------------------------------------------------------------
# backward flags.  A discriminator forward on generated frames serves two losses: the discriminator's
# (gradients for the discriminator parameters only) and the generator's (gradients for the frames
# only).  The reference runs that forward twice -- netD(fake.detach()) and netD(fake) with the result of
# the latter never reaching optimizer_D (discriminator.py:154-166) -- although both produce the same
# activations.  Here it runs once; which gradients a backward pass over it produces is selected by
# flags the trainer sets on the convolution modules around each loss.backward():
#   SKIP_PARAM_GRADS  no weight / bias / BatchNorm gradients (the generator's pass)
#   SKIP_INPUT_GRAD   an input layer ('first' stage) returns no gradient for the image (the
#                     discriminator's pass: nothing flows back into the generator)
# ---------------------------------------------------------------------------------------------
SKIP_PARAM_GRADS, SKIP_INPUT_GRAD = 1, 2
FUSED_BN = os.environ.get("IR2RGB_FUSED_BN", "1") != "0"    # bn_finalize + bn_apply in one launch where the statistics are few rows


@contextlib.contextmanager
def backward_flags(modules, flags, active_groups=None):
    """For the backward passes run inside: ``flags`` (SKIP_*) on every convolution stage of ``modules``; ``active_groups``
    = k: of the sample groups of a batched forward (conv_stage(groups=G)) only the first k receive a gradient in this
    pass -- the stages then work on that leading part of the batch only and leave the rest of every gradient tensor
    unwritten (nobody reads it: the generator's pass through the discriminators never reaches the real frames)."""
    convs = [m for mod in modules for m in mod.modules() if isinstance(m, (torch.nn.Conv2d, torch.nn.ConvTranspose2d))]
    for m in convs:
        m._ir2rgb_bwd = flags
        m._ir2rgb_active = active_groups
    try:
        yield
    finally:
        for m in convs:
            m._ir2rgb_bwd = 0
            m._ir2rgb_active = None


# ---------------------------------------------------------------------------------------------
# the fused stage
# ---------------------------------------------------------------------------------------------
def _fused_act(spec):
    """Activation fused into the convolution epilogue of a stage WITHOUT BatchNorm (ir2rgb_conv_desc.act)."""
    return 1 if spec["fused_leaky"] else (3 if spec.get("fused_relu") else 0)


def _group(t, g, G):
    """Sample group ``g`` of ``G`` in a tensor batched along its first dimension (activations: N / G samples; a
    convolution's per-sample statistics: rows / G partial rows)."""
    n = t.shape[0] // G
    return t[g * n:(g + 1) * n]


def _stage_geometry(spec, conv, x, bias, per_sample_stats):
    """What the stage's convolution launch reads: -> (xin, descriptor, packed weight, bias, weight_fn, sub-spec).  The only
    place that knows how a first layer (x-im2col of the fp32 image + a (kh x 1) convolution, whose spec is the sub-spec)
    and a layer at padded widths differ from the plain one.  ``weight_fn`` maps conv.weight to the weight the launch
    uses (None: the parameter itself); the bias comes back zero-padded to the width the layer runs at."""
    dt = spec["dtype"]
    cout, cin = conv.out_channels, conv.in_channels
    cout_p = cout if spec.get("out_f32", False) else padded_width(cout)
    cin_p = cin if spec["first"] else padded_width(cin)
    padded = cout_p != cout or cin_p != cin
    wfn = _pad_weight_fn(cout_p, cin_p, spec["transposed"]) if padded else None
    if spec["first"]:
        kh, kw = conv.kernel_size
        sub = dict(spec, k=(kh, 1), stride=(spec["stride"][0], 1), pad=(spec["pad"][0], 0))
        xin = L.xexpand(x, kw, spec["stride"][1], spec["pad"][1], spec["pad_mode"], dt)
        desc = C.make_desc(tuple(xin.shape), cout_p, sub["k"], sub["stride"], sub["pad"], spec["pad_mode"], dt,
                           act=_fused_act(spec))
        wfn = _compose(wfn, L._xexpanded_weight(kw))
        wp = L.packed_weight(conv, desc, wfn, tag="xexp")
    else:
        if x.shape[1] != cin_p:
            raise ValueError(f"conv stage: input has {x.shape[1]} channels, the layer runs at {cin_p} (autograd.pad_channels)")
        xin, sub = x, None
        desc = C.make_desc(tuple(x.shape), cout_p, spec["k"], spec["stride"], spec["pad"], spec["pad_mode"],
                           dt, spec["transposed"], spec.get("output_padding", 0), act=_fused_act(spec),
                           out_f32=spec.get("out_f32", False), stats_per_sample=per_sample_stats)
        wp = L.packed_weight(conv, desc, wfn, tag="wpad" if padded else "w")
    if padded and bias is not None:
        bias = L.pad_dim(bias.detach(), 0, cout_p)
    return xin, desc, wp, bias, wfn, sub


def _batchnorm(spec, bn, y, stats, bias, res1, res2, frozen):
    """BatchNorm + activation (+ residuals) of the convolution output ``y``: -> (z, scale, shift, mean, invstd), the four
    vectors [C], or [G][C] for a batch of G sample groups."""
    G = spec.get("groups", 1)
    n, ch, h, w = y.shape
    count = n * h * w // G
    fused = FUSED_BN and not frozen and spec["training"] and ch % 64 == 0
    if G == 1:
        if fused and stats.shape[0] <= L.FUSED_BN_MAX_ROWS:
            # few partial rows (the residual blocks): statistics and apply in one launch
            return L.bn_finalize_apply(stats, count, bn, y, spec["act"], res1, res2, bias)
        scale, shift, mean, invstd = L.bn_finalize(stats, count, bn, spec["training"], bias)
        return L.bn_apply(y, scale, shift, spec["act"], res1, res2), scale, shift, mean, invstd
    # G independent forwards batched along N (the discriminators see real / generated / raw frames with the same
    # weights): ONE convolution, then BatchNorm per sample group exactly as G separate calls would run it --
    # statistics over the group's samples, running statistics advanced group by group
    if n % G or res1 is not None or res2 is not None:
        raise ValueError("conv stage: sample groups need N % groups == 0 and no residual inputs")
    rg = 0 if frozen else stats.shape[0] // G
    z = torch.empty_like(y, memory_format=torch.channels_last)
    vec = torch.empty((4, G, ch), dtype=torch.float32, device=y.device)
    reps = L._STAT_UPDATES        # layers.repeated_forward: an int, or one count per group
    try:
        for g in (spec.get("group_order") or range(G)):      # (the order the running statistics advance in)
            L._STAT_UPDATES = reps[g] if isinstance(reps, tuple) else reps
            yg, zg = _group(y, g, G), _group(z, g, G)
            sg = None if frozen else _group(stats, g, G)
            outs = (vec[0][g], vec[1][g], vec[2][g], vec[3][g])
            if fused and rg <= L.FUSED_BN_MAX_ROWS:
                L.bn_finalize_apply(sg, count, bn, yg, spec["act"], None, None, bias, out=zg, outs=outs)
            else:
                L.bn_finalize(sg, count, bn, spec["training"], bias, outs=outs)
                L.bn_apply(yg, outs[0], outs[1], spec["act"], out=zg)
    finally:
        L._STAT_UPDATES = reps
    return z, vec[0], vec[1], vec[2], vec[3]


def _bn_grad(gz, y, scale, shift, mean, invstd, act):
    """BatchNorm + activation backward, per sample group where the vectors are [G][C] (into one gradient tensor for the
    batch, the parameter gradients summed over the groups): -> (gy, dgamma, dbeta)."""
    if scale.dim() == 1:
        return bn_bwd(gz, y, scale, shift, mean, invstd, act)
    G = scale.shape[0]
    gy = torch.empty_like(y, memory_format=torch.channels_last)
    params = None
    for g in range(G):
        _, dgamma, dbeta = bn_bwd(_group(gz, g, G), _group(y, g, G), scale[g], shift[g], mean[g], invstd[g], act,
                                  out=_group(gy, g, G), params=params)
        params = (dgamma, dbeta)
    return gy, dgamma, dbeta


def _output_grad(ctx, gz, y, scale, shift, mean, invstd):
    """Back through activation / BatchNorm / the fp32 cast to the convolution output: -> (gz as the residual branches get it,
    gy for the data gradient, gy for the weight gradient, dbias, dgamma, dbeta)."""
    spec = ctx.spec
    hdt = spec["dtype"]
    if spec.get("out_f32", False):
        # thin fp32 output (PatchGAN logits): the gradient zero-padded to 64 channels for the MFMA adjoint and to 8 for
        # the weight-gradient kernel, and its per-channel sum, in one launch
        g64, g8, dbias = thin_grad_expand(gz, hdt)
        return gz, g64, g8, dbias, None, None
    gz = _as_half_nhwc(gz, hdt)
    if ctx.has_bn:
        gy, dgamma, dbeta = _bn_grad(gz, y, scale, shift, mean, invstd, spec["act"] | (BN_BWD_FROZEN if ctx.frozen else 0))
        # training mode: BatchNorm removes the per-channel mean, the bias gradient is exactly 0 (None = zeros);
        # evaluation mode: the layer is affine in the bias, d/dbias = scale * sum g' (the same running statistics for
        # every sample group)
        dbias = dbeta * (scale if scale.dim() == 1 else scale[0]) if ctx.frozen else None
        return gz, gy, gy, dbias, dgamma, dbeta
    # LeakyReLU / ReLU keep the sign (ReLU: y > 0 <=> pre-activation > 0): mask from the stored output
    act = 2 if spec["fused_leaky"] else (1 if spec.get("fused_relu") else 0)
    gy, _, dbias = bn_bwd(gz, y, None, None, None, None, act)
    return gz, gy, gy, dbias, None, None


def _image_grad(ctx, gy, xin):
    """Input gradient of a first layer (NCHW fp32): the adjoint of the (kh x 1) convolution over the expanded image, then
    of the x-im2col."""
    spec, conv = ctx.spec, ctx.conv
    if spec["pad_mode"] != C.PAD_ZERO:
        raise NotImplementedError("input gradient of a reflect-padded first layer is never needed")
    kw = conv.kernel_size[1]
    dxe = conv_dgrad(gy, conv, ctx.sub, tuple(xin.shape), ctx.wfn, tag="dgrad_xexp")
    return xexpand_bwd(dxe, ctx.x_shape[1], ctx.x_shape[3], kw, spec["stride"][1], spec["pad"][1], spec["pad_mode"])


def _input_grad(ctx, gy, xin, n_full):
    """Gradient w.r.t. the stage's input.  ``n_full``: the forward's batch size when ``gy`` covers its leading samples only
    -- the gradient keeps the full batch's shape and the rest of it stays unwritten."""
    spec, conv = ctx.spec, ctx.conv
    if spec["first"]:
        dx = _image_grad(ctx, gy, xin)
        if n_full is not None:
            full = dx.new_empty((n_full,) + tuple(dx.shape[1:]))
            full[:dx.shape[0]].copy_(dx)
            dx = full
        return dx
    wfn = ctx.wfn
    if gy.shape[1] != ctx.width:       # a gradient widened for the MFMA kernel (thin outputs): zero weight rows to match
        wfn = _compose(wfn, lambda w: L.pad_dim(w, 0, gy.shape[1]))
    if n_full is None:
        return conv_dgrad(gy, conv, spec, ctx.x_shape, wfn)
    dx = C.empty_nhwc(n_full, ctx.x_shape[1], ctx.x_shape[2], ctx.x_shape[3], gy.dtype, gy.device)
    conv_dgrad(gy, conv, spec, (gy.shape[0],) + tuple(ctx.x_shape[1:]), wfn, out=dx[:gy.shape[0]])
    return dx


def _weight_grad(ctx, xin, gy):
    """Gradient of conv.weight, in the parameter's own shape, from the launch's input and the gradient w.r.t. its output."""
    spec, conv = ctx.spec, ctx.conv
    cout, cin = conv.out_channels, conv.in_channels
    if spec["first"]:
        kh, kw = conv.kernel_size

        def wgrad():
            gwe = conv_wgrad(xin, gy, None, ctx.sub)                            # [co_p][64][kh][1]
            gwe = gwe[:cout, :cin * kw, :, 0].reshape(cout, cin, kw, kh)        # [co][ci][kx][ky]
            return gwe.permute(0, 1, 3, 2).contiguous()
    elif gy.shape[1] != cout or xin.shape[1] != cin:
        # the launch ran wider than the parameter (padded widths; a thin gradient zero-padded to 8 channels): the
        # parameter's gradient is the real corner
        def wgrad():
            g = conv_wgrad(xin, gy, None, spec)
            return (g[:cin, :cout] if spec["transposed"] else g[:cout, :cin]).contiguous()
    else:
        wsh = tuple(conv.weight.shape)
        out, acc, dw = wgrad_destination(conv.weight, wsh)
        if acc:
            conv_wgrad(xin, gy, wsh, spec, out=out, accumulate=True)
            return dw

        def wgrad():            # (conv2d_wgrad hands back the fresh tensor, or its own new view of the sink)
            g = conv_wgrad(xin, gy, wsh, spec, out=out)
            if SC.ENABLED and out is not None:
                SC.produced(out, f"grad sink {wsh}")
            return g
    return wgrad_overlapped(conv, wgrad, xin, gy)


class ConvStageFn(Function):
    """z = act(bn(conv(x))) + res1 + res2 on channels_last half tensors (x may be an NCHW fp32 image
    for 'first' stages).  Arguments after ``x``: weight, bias, gamma, beta (fp32 parameters), res1,
    res2, then the non-tensor ``spec`` dict and the conv / bn modules (packed-weight cache, BN
    buffers).  The plain stage runs from its cached plan (ir2rgb_amd/stageplan.py); everything else through the steps
    above, which make the same library calls."""

    @staticmethod
    def forward(ctx, x, weight, bias, gamma, beta, res1, res2, spec, conv, bn):
        plan = stageplan.lookup(x, spec, conv, bn, FUSED_BN)
        if plan is not None:        # the plain stage, host work precomputed (ir2rgb_amd/stageplan.py): same launches
            return plan.forward(ctx, x, bias, res1, res2, conv, bn)
        ctx.plan = None
        xin, desc, wp, bias, ctx.wfn, ctx.sub = _stage_geometry(spec, conv, x, bias,
                                                                bn is not None and spec.get("groups", 1) > 1)
        scale = shift = mean = invstd = None
        ctx.frozen = False
        if bn is None:
            y, _ = C.conv2d_fwd(desc, xin, wp, bias)
            z = y
        else:
            # the bias of a convolution in front of BatchNorm cancels: it is left out of the activations and
            # handed to the statistics kernel, which needs it for the running mean only (ir2rgb_bn_finalize_ex)
            ctx.frozen = L.bn_frozen(bn, spec["training"])
            y, stats = C.conv2d_fwd(desc, xin, wp, None, want_stats=not ctx.frozen)
            bnp = _PaddedBN(bn, desc.Cout) if desc.Cout != conv.out_channels else bn
            z, scale, shift, mean, invstd = _batchnorm(spec, bnp, y, stats, bias, res1, res2, ctx.frozen)
            if bnp is not bn:
                bnp.commit(spec["training"])
        ctx.spec, ctx.conv = spec, conv
        ctx.x_shape, ctx.width = tuple(x.shape), desc.Cout
        ctx.has_bn = bn is not None
        ctx.has_res = (res1 is not None, res2 is not None)
        ctx.save_for_backward(xin, y, scale, shift, mean, invstd)
        return z

    @staticmethod
    def backward(ctx, gz):
        plan = ctx.plan
        if plan is not None:        # (the plan honours the backward flags and inactive sample groups itself)
            return plan.backward(ctx, gz)
        spec, conv = ctx.spec, ctx.conv
        xin, y, *bnv = ctx.saved_tensors            # bnv: scale, shift, mean, invstd
        flags = getattr(conv, "_ir2rgb_bwd", 0)
        want_params = not (flags & SKIP_PARAM_GRADS)
        want_dx = ctx.needs_input_grad[0] and not (spec["first"] and (flags & SKIP_INPUT_GRAD))
        # sample groups of which only the leading k carry a gradient in this pass (backward_flags): work on that part
        G, k = spec.get("groups", 1), getattr(conv, "_ir2rgb_active", None)
        n_full = None
        if G > 1 and k is not None and k < G:
            if want_params:
                raise RuntimeError("conv stage: a pass with inactive sample groups cannot produce parameter gradients")
            n_full = y.shape[0]
            na = n_full // G * k
            gz, y, xin = gz[:na], y[:na], xin[:na]
            if bnv[0] is not None and bnv[0].dim() == 2:
                bnv = [v[:k] for v in bnv]
        gz, gy, gyw, dbias, dgamma, dbeta = _output_grad(ctx, gz, y, *bnv)
        dx = _input_grad(ctx, gy, xin, n_full) if want_dx else None
        dw = None
        if not want_params:
            dbias = dgamma = dbeta = None
        elif ctx.needs_input_grad[1]:
            dw = _weight_grad(ctx, xin, gyw)
        if ctx.width != conv.out_channels:      # padded width: reference-shaped parameter gradients
            dbias, dgamma, dbeta = (None if t is None else t[:conv.out_channels] for t in (dbias, dgamma, dbeta))
        r1 = gz if ctx.has_res[0] else None
        r2 = gz if ctx.has_res[1] else None
        return dx, dw, (dbias if ctx.needs_input_grad[2] else None), dgamma, dbeta, r1, r2, None, None, None


def conv_stage(x, conv, bn, act, pad_mode, dtype, *, first=False, stride=None, pad=None, transposed=False,
               output_padding=0, res1=None, res2=None, fused_leaky=False, training=True, out_f32=False, fused_relu=False,
               groups=1, group_order=None):
    """Autograd-aware stage: act(bn(conv(x))) + res1 + res2 (bn may be None).  ``groups`` > 1: the batch holds that many
    independent forwards (N / groups samples each) -- BatchNorm treats them as separate calls."""
    stride = tuple(conv.stride) if stride is None else C._pair(stride)
    pad = tuple(conv.padding) if pad is None else C._pair(pad)
    spec = dict(k=tuple(conv.kernel_size), stride=stride, pad=pad, pad_mode=pad_mode, transposed=transposed,
                output_padding=output_padding, act=act, fused_leaky=fused_leaky, fused_relu=fused_relu, training=training, dtype=dtype,
                first=first, out_f32=out_f32, groups=groups, group_order=group_order)
    gamma = bn.weight if bn is not None else None
    beta = bn.bias if bn is not None else None
    return ConvStageFn.apply(x, conv.weight, conv.bias, gamma, beta, res1, res2, spec, conv, bn)


# ---------------------------------------------------------------------------------------------
# heads, warp-blend and the small element-wise stages: HIP forward and HIP backward
# ---------------------------------------------------------------------------------------------
class HeadFn(Function):
    """Separable 7x7 head(s) on one feature map: HIP forward (1x7 MFMA pass + head_finish) and HIP
    backward (head_finish_bwd -> adjoint 1x7 MFMA convolution + reflect fold for the feature gradient,
    MFMA wgrad for the kernels)."""

    @staticmethod
    def forward(ctx, feat, acts, mul, convs, *params):
        out = L.head_stage(feat, convs, acts, mul)
        ctx.acts, ctx.mul, ctx.convs = acts, mul, convs
        ctx.save_for_backward(feat, out)
        return out

    @staticmethod
    def backward(ctx, gout):
        feat, out = ctx.saved_tensors
        convs, acts, mul = ctx.convs, ctx.acts, ctx.mul
        kh, kw = convs[0].kernel_size
        n, cin, h, w = feat.shape
        cout = out.shape[1]
        CT = 64
        gout = gout.float().contiguous()
        dT = C.empty_nhwc(n, CT, h, w, feat.dtype, feat.device)
        dbias = torch.empty(cout, dtype=torch.float32, device=feat.device)
        partial = torch.empty((_lib.query("ir2rgb_head_finish_bwd_rows", n, h, w), 8), dtype=torch.float32, device=feat.device)
        _lib.launch("ir2rgb_head_finish_bwd", feat, gout, out, dT, dbias, partial, n, h, w, cout, kh, CT, kh // 2,
                    L.pack_acts(acts), float(mul), _DT[feat.dtype])
        gfeat = None
        if ctx.needs_input_grad[0]:
            desc = C.make_desc((n, CT, h, w), cin, (1, kw), 1, (0, kw - 1), C.PAD_ZERO, feat.dtype)
            # the adjoint packing of the [64][cin][1][kw] forward weight
            dpad, _ = C.conv2d_fwd(desc, dT, L.head_weight(convs, desc, cin, rows=CT, adjoint=True))
            gfeat = fold_reflect(dpad, 0, kw // 2)
        wdesc = C.make_desc(tuple(feat.shape), CT, (1, kw), 1, (0, kw // 2), C.PAD_REFLECT, feat.dtype)
        gw = C.conv2d_wgrad(wdesc, feat, dT)                                       # [64][cin][1][kw]
        gw = gw[:cout * kh, :, 0, :].reshape(cout, kh, cin, kw).permute(0, 2, 1, 3)                 # [cout][cin][kh][kw]
        gw = gw[:, :convs[0].in_channels].contiguous()          # (a padded feature map: the real input channels)
        gws, gbs, o = [], [], 0
        for c in convs:
            gws.append(gw[o:o + c.out_channels])
            gbs.append(dbias[o:o + c.out_channels])
            o += c.out_channels
        return (gfeat, None, None, None) + tuple(gws) + tuple(gbs)


def head_stage(feat, convs, acts, mul=1.0):
    params = [c.weight for c in convs] + [c.bias for c in convs]
    return HeadFn.apply(feat, list(acts), float(mul), list(convs), *params)


class WarpBlendFn(Function):
    """img_final = raw*w + warp(prev, flow)*(1-w): HIP forward and HIP backward w.r.t. raw, flow, w.
    A gradient w.r.t. prev (never needed on the training path: prev is detached, generator.py:153-154)
    falls back to torch autograd of the same formula."""

    @staticmethod
    def forward(ctx, raw, prev, flow, weight):
        raw, prev, flow, weight = raw.contiguous(), prev.contiguous(), flow.contiguous(), weight.contiguous()
        ctx.save_for_backward(raw, prev, flow, weight)
        return L.warp_blend(raw, prev, flow, weight)

    @staticmethod
    def backward(ctx, gout):
        raw, prev, flow, weight = ctx.saved_tensors
        gout = gout.float().contiguous()
        graw, gflow, gw = torch.empty_like(raw), torch.empty_like(flow), torch.empty_like(weight)
        n, _, h, w = raw.shape
        _lib.launch("ir2rgb_warp_blend_bwd", raw, gout, raw, prev, flow, weight, graw, gflow, gw, n, prev.shape[1], h, w)
        gprev = None
        if ctx.needs_input_grad[1]:
            from .networks import get_grid
            with torch.enable_grad():
                p = prev.detach().requires_grad_()
                grid = get_grid(n, h, w, device=raw.device, dtype=flow.dtype)
                fln = torch.cat([flow[:, 0:1] / ((w - 1.0) / 2.0), flow[:, 1:2] / ((h - 1.0) / 2.0)], 1)
                warp = F.grid_sample(p[:, -3:], (grid + fln).permute(0, 2, 3, 1), mode="bilinear", padding_mode="border",
                                     align_corners=False)
                gprev, = torch.autograd.grad(warp, p, gout * (1 - weight))
        return graw, gprev, gflow, gw


def warp_blend(raw, prev, flow, weight):
    return WarpBlendFn.apply(raw, prev, flow, weight)


class AvgPool3s2Fn(Function):
    """AvgPool2d(3, stride 2, padding 1, count_include_pad=False) of an fp32 [..., H, W] tensor (ir2rgb_avgpool3s2)."""

    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        h, w = x.shape[-2:]
        ctx.shape = tuple(x.shape)
        y = torch.empty(tuple(x.shape[:-2]) + ((h - 1) // 2 + 1, (w - 1) // 2 + 1), dtype=torch.float32, device=x.device)
        _lib.launch("ir2rgb_avgpool3s2", x, x, y, x.numel() // (h * w), h, w, 0)
        return y

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        gx = torch.empty(ctx.shape, dtype=torch.float32, device=g.device)
        h, w = ctx.shape[-2:]
        _lib.launch("ir2rgb_avgpool3s2", g, g, gx, gx.numel() // (h * w), h, w, 1)
        return gx


def avg_pool3s2(x):
    """The pyramids' down-sampling step; torch's operator for anything but fp32 GPU tensors."""
    if x.is_cuda and x.dtype == torch.float32 and x.dim() >= 2:
        return AvgPool3s2Fn.apply(x)
    return torch.nn.functional.avg_pool2d(x, 3, stride=2, padding=1, count_include_pad=False)


class AddFn(Function):
    """a + b on channels_last half tensors (HIP), gradient passed to both."""

    @staticmethod
    def forward(ctx, a, b):
        return L.bn_apply_add(a, b)

    @staticmethod
    def backward(ctx, g):
        return g, g


def add(a, b):
    return AddFn.apply(a, b)


class ToHalfFn(Function):
    """NCHW fp32 (or any) -> channels_last half (HIP converter); backward converts the gradient back."""

    @staticmethod
    def forward(ctx, x, dtype):
        ctx.src_dtype = x.dtype
        return L.to_nhwc_half(x, dtype)

    @staticmethod
    def backward(ctx, g):
        return (L.to_nchw_f32(g) if ctx.src_dtype == torch.float32 else g.to(ctx.src_dtype)), None


def to_nhwc_half(x, dtype):
    if x.dtype == dtype and C.is_nhwc(x):
        return x
    return ToHalfFn.apply(x, dtype)
