"""FlowNet2's convolution stacks on the hand-written MFMA kernels (SURVEY section 8 "next" row f1).

Executes the parameter tree of ``ir2rgb_amd.flownet2_pytorch.models.FlowNet2`` (same module names
as reference models/flownet2_pytorch/networks/{FlowNetC,FlowNetS,FlowNetSD,FlowNetFusion}.py) with
``ir2rgb_conv2d_fwd``: every ``conv(...)+LeakyReLU(0.1)``, ``deconv`` (ConvTranspose 4x4 s2),
``i_conv`` and ``predict_flow`` becomes one launch with the activation fused, and every ``torch.cat``
of the refinement decoders disappears: producers write straight into channel slices of NHWC
concatenation buffers (ir2rgb_conv_desc.ldy / co_off) and consumers read slices (ldx / ci_off).
Concatenation widths that are not multiples of 64 (473, 1026, 770, 386, 194, 162, 82) are padded with
zero channels in the buffer and zero columns in the packed weights.

The 2-channel ConvTranspose2d(2,2,4,2,1) flow up-samplers are a small direct kernel writing into the
same buffers.  Left on torch (tiny 2..12-channel fp32 tensors): the x4 interpolations and the
normalisation / concatenation glue of FlowNet2.forward.
"""
import os

import torch

from . import _lib
from . import conv as C
from . import layers as L

LEAKY01 = 2  # ir2rgb_conv_desc.act code for LeakyReLU(0.1)


def _up64(c):
    return (c + 63) // 64 * 64


class View:
    """Channels [off, off+ch) of an NHWC half buffer ``buf`` (logical [N, ld, H, W], channels_last)."""

    def __init__(self, buf, off, ch):
        self.buf, self.off, self.ch = buf, off, ch

    @property
    def n(self):
        return self.buf.shape[0]

    @property
    def ld(self):
        return self.buf.shape[1]

    @property
    def hw(self):
        return self.buf.shape[2], self.buf.shape[3]


class _Run:
    """One call of a sub-network: its batch, dtype and device, and the pool of NHWC buffers of (net, input shape, dtype,
    device), allocated and zero-filled on the first such call and handed out in call order after that.  Pad channels are
    never written, so they stay zero across calls; every real channel is overwritten by its producer on each forward.
    Pools live ON the sub-network module (not in a table keyed by id(net): ids are recycled once a network is garbage
    collected)."""

    def __init__(self, net, x, dtype):
        self.n, self.dtype, self.device, self.cursor = x.shape[0], dtype, x.device, 0
        self.pool = net.__dict__.setdefault("_ir2rgb_workspaces", {}).setdefault((tuple(x.shape), dtype, x.device), [])

    def buf(self, ld, h, w):
        shape = (self.n, ld, h, w)
        if self.cursor == len(self.pool):
            self.pool.append(torch.zeros(shape, dtype=self.dtype, device=self.device).contiguous(memory_format=torch.channels_last))
        b = self.pool[self.cursor]
        if tuple(b.shape) != shape:
            raise RuntimeError("FlowNet2 workspace: allocation sequence changed")
        self.cursor += 1
        return b

    def conv_out(self, mod, hw):
        """A buffer of its own for the result of the nn.Conv2d ``mod`` on an input of size ``hw``, as a View."""
        h, w = ((s + 2 * p - k) // st + 1 for s, k, st, p in zip(hw, mod.kernel_size, mod.stride, mod.padding))
        return View(self.buf(_up64(mod.out_channels), h, w), 0, mod.out_channels)


def _pad_cin(cin_to, transposed):
    return lambda w: L.pad_dim(w, 0 if transposed else 1, cin_to)


def conv(xv, mod, yv, act, *, k=None, stride=None, pad=None, transposed=False, out_f32=False, weight_fn=None, tag="fn"):
    """yv <- act(conv(xv)).  xv / yv are Views; ``mod`` an nn.Conv2d / nn.ConvTranspose2d (weights, bias)."""
    k = tuple(mod.kernel_size) if k is None else k
    stride = tuple(mod.stride) if stride is None else stride
    pad = tuple(mod.padding) if pad is None else pad
    n = xv.n
    h, w = xv.hw
    cin = _up64(xv.ch)
    if xv.off + cin > xv.ld:
        raise ValueError("input view: padded channel range exceeds the buffer")
    dt = xv.buf.dtype
    cout = yv.ch
    oh, ow = yv.hw
    desc = C.ConvDesc(n, h, w, cin, oh, ow, cout, k[0], k[1], stride[0], stride[1], pad[0], pad[1], C.PAD_ZERO,
                      int(transposed), C._TORCH2DT[dt], act, int(out_f32), xv.ld, xv.off, yv.ld, yv.off)
    fn = _pad_cin(cin, transposed) if weight_fn is None else weight_fn
    wp = L.packed_weight(mod, desc, fn, tag=tag)
    C.conv2d_fwd_view(desc, xv.buf, wp, mod.bias, yv.buf)
    return yv


def first_conv(x_nchw, mod, yv, dtype):
    """Small-Cin first layer (7x7 s2 on 3/12 channels, 3x3 on 6/11): x-im2col + (kh x 1) MFMA convolution."""
    kh, kw = mod.kernel_size
    sh, sw = mod.stride
    ph, pw = mod.padding
    cx = 64 if mod.in_channels * kw <= 64 else 128
    xe = L.xexpand(x_nchw, kw, sw, pw, C.PAD_ZERO, dtype, cx=cx)
    return conv(View(xe, 0, cx), mod, yv, LEAKY01, k=(kh, 1), stride=(sh, 1), pad=(ph, 0),
                weight_fn=L._xexpanded_weight(kw, cx), tag="fn_xexp")


def put_nchw(x_nchw, yv, act=0):
    """NCHW fp32 -> channel slice of an NHWC half buffer (optionally LeakyReLU(0.1))."""
    x = x_nchw.float().contiguous()
    n, c, h, w = x.shape
    _lib.launch("ir2rgb_nchw_f32_to_nhwc_half_slice", x, x, yv.buf, n, c, h, w, yv.ld, yv.off, act, C._TORCH2DT[yv.buf.dtype])


def corr_nhwc(mod, av, bv, yv, slope):
    """FlowNetC's cost volume (Correlation(20, 1, 20, 1, 2), FlowNetC.py:27) + LeakyReLU straight from the two NHWC half
    feature maps into a channel slice of ``yv.buf`` (ir2rgb_correlation_nhwc_half: banded MFMA products).  False when the
    operator's parameters or the shape are outside what that kernel covers."""
    cfg = tuple(getattr(mod, k, None) for k in ("pad_size", "kernel_size", "max_displacement", "stride1", "stride2"))
    if cfg != (20, 1, 20, 1, 2) or getattr(mod, "corr_multiply", 1) != 1 or yv.ch != 441 or av.ch != bv.ch:
        return False
    if os.environ.get("IR2RGB_CORR_MFMA", "1") == "0":
        return False
    n = av.n
    h, w = av.hw
    with _lib.on_device(av.buf):        # (explicit, not _lib.launch: "not supported" is an answer here, not an error)
        rc = _lib.lib().ir2rgb_correlation_nhwc_half(av.buf, av.ld, av.off, bv.buf, bv.ld, bv.off, yv.buf, 1, yv.ld,
                                                     yv.off, float(slope), n, av.ch, h, w, C._TORCH2DT[av.buf.dtype],
                                                     _lib.current_stream(av.buf))
    if rc == _lib.IR2RGB_ENOSUP:
        return False
    _lib.check(rc, "correlation_nhwc_half")
    return True


def flow_up(flow, mod, yv):
    """ConvTranspose2d(2,2,4,2,1) of a 2-channel fp32 flow, written into a 2-channel slice of ``yv.buf``."""
    n, _, h, w = flow.shape
    _lib.launch("ir2rgb_flow_upsample_slice", flow, flow, mod.weight, mod.bias, yv.buf, n, h, w, yv.ld, yv.off,
                C._TORCH2DT[yv.buf.dtype])


def predict(xv, mod, n, h, w):
    """predict_flow (3x3, 2 channels): fp32 NCHW [N,2,h,w]."""
    out = torch.empty((n, 2, h, w), dtype=torch.float32, device=xv.buf.device).contiguous(memory_format=torch.channels_last)
    conv(xv, mod, View(out, 0, 2), 0, out_f32=True)
    return out.contiguous()


class _Decoder:
    """Coarse-to-fine refinement shared by FlowNetC / FlowNetS / FlowNetSD: levels 6 -> 2."""
    SKIP = {5: 512, 4: 512, 3: 256, 2: 128}
    DEC = {5: 512, 4: 256, 3: 128, 2: 64}

    def __init__(self, ctx, h6, w6):
        self.ctx = ctx
        self.cat = {lvl: ctx.buf(_up64(self.SKIP[lvl] + self.DEC[lvl] + 2), h6 << (6 - lvl), w6 << (6 - lvl)) for lvl in (5, 4, 3, 2)}

    def skip_view(self, lvl):
        return View(self.cat[lvl], 0, self.SKIP[lvl])

    def full_view(self, lvl):
        return View(self.cat[lvl], 0, self.SKIP[lvl] + self.DEC[lvl] + 2)

    def encode(self, net, x, levels):
        """convK -> convK_1 for each level K of ``levels``; level K's result is the skip slice of its concatenation buffer
        (level 6, which has none: a dense buffer)."""
        for lvl in levels:
            a, b = getattr(net, f"conv{lvl}")[0], getattr(net, f"conv{lvl}_1")[0]
            x = conv(x, a, self.ctx.conv_out(a, x.hw), LEAKY01)
            x = conv(x, b, self.skip_view(lvl) if lvl in self.cat else self.ctx.conv_out(b, x.hw), LEAKY01)
        return x

    def run(self, net, feat6, inter=False):
        n = feat6.n
        feat, flow_in = feat6, feat6
        for lvl in (6, 5, 4, 3):
            h, w = feat.hw
            flow = predict(flow_in, getattr(net, f"predict_flow{lvl}"), n, h, w)
            nxt = self.cat[lvl - 1]
            so, do = self.SKIP[lvl - 1], self.DEC[lvl - 1]
            conv(feat, getattr(net, f"deconv{lvl - 1}")[0], View(nxt, so, do), LEAKY01, transposed=True)
            flow_up(flow, getattr(net, f"upsampled_flow{lvl}_to_{lvl - 1}"), View(nxt, so + do, 2))
            feat = self.full_view(lvl - 1)
            if inter:
                ic = getattr(net, f"inter_conv{lvl - 1}")[0]
                flow_in = conv(feat, ic, self.ctx.conv_out(ic, feat.hw), 0)
            else:
                flow_in = feat
        h, w = feat.hw
        return predict(flow_in, net.predict_flow2, n, h, w)


def _begin(net, x, dtype):
    """-> (run context, decoder) of one FlowNetC / S / SD call on ``x`` [N, C, H, W], H and W multiples of 64."""
    ctx = _Run(net, x, dtype)
    return ctx, _Decoder(ctx, x.shape[2] // 64, x.shape[3] // 64)


def flownetc(net, x, dtype):
    """x [N,6,H,W] fp32 (two normalised images) -> flow2 [N,2,H/4,W/4] fp32 (reference FlowNetC.py:75-126)."""
    ctx, dec = _begin(net, x, dtype)
    feats = []
    for img, skip in ((x[:, 0:3], True), (x[:, 3:6], False)):
        c1 = first_conv(img, net.conv1[0], ctx.conv_out(net.conv1[0], img.shape[2:]), dtype)
        c2 = conv(c1, net.conv2[0], dec.skip_view(2) if skip else ctx.conv_out(net.conv2[0], c1.hw), LEAKY01)
        feats.append(conv(c2, net.conv3[0], ctx.conv_out(net.conv3[0], c2.hw), LEAKY01))
    a3, b3 = feats
    merged = ctx.buf(512, *a3.hw)                                                  # [redir 32 | corr 441 | pad]
    conv(a3, net.conv_redir[0], View(merged, 0, 32), LEAKY01)
    if not corr_nhwc(net.corr, a3, b3, View(merged, 32, 441), 0.1):                # MFMA cost volume + corr_activation
        cost = net.corr(L.to_nchw_f32(a3.buf), L.to_nchw_f32(b3.buf))             # (shapes it does not cover: scalar kernel, fp32)
        put_nchw(cost, View(merged, 32, 441), act=LEAKY01)
    c3 = conv(View(merged, 0, 473), net.conv3_1[0], dec.skip_view(3), LEAKY01)
    return dec.run(net, dec.encode(net, c3, (4, 5, 6)))


def flownets(net, x, dtype):
    """x [N,12,H,W] fp32 -> flow2 (reference FlowNetS.py:57-93)."""
    ctx, dec = _begin(net, x, dtype)
    c1 = first_conv(x, net.conv1[0], ctx.conv_out(net.conv1[0], x.shape[2:]), dtype)
    c2 = conv(c1, net.conv2[0], dec.skip_view(2), LEAKY01)
    return dec.run(net, dec.encode(net, c2, (3, 4, 5, 6)))


def flownetsd(net, x, dtype):
    """x [N,6,H,W] fp32 -> flow2 (reference FlowNetSD.py:66-105)."""
    ctx, dec = _begin(net, x, dtype)
    c0 = first_conv(x, net.conv0[0], ctx.conv_out(net.conv0[0], x.shape[2:]), dtype)
    c1 = conv(c0, net.conv1[0], ctx.conv_out(net.conv1[0], c0.hw), LEAKY01)
    c1 = conv(c1, net.conv1_1[0], ctx.conv_out(net.conv1_1[0], c1.hw), LEAKY01)
    return dec.run(net, dec.encode(net, c1, (2, 3, 4, 5, 6)), inter=True)


def flownetfusion(net, x, dtype):
    """x [N,11,H,W] fp32 -> flow0 [N,2,H,W] (reference FlowNetFusion.py:47-66)."""
    ctx = _Run(net, x, dtype)
    n, _, H, W = x.shape
    cat0 = ctx.buf(128, H, W)            # [conv0 64 | deconv0 16 | flow1_up 2 | pad]
    cat1 = ctx.buf(192, H // 2, W // 2)  # [conv1 128 | deconv1 32 | flow2_up 2 | pad]
    c0 = first_conv(x, net.conv0[0], View(cat0, 0, 64), dtype)
    c1 = conv(conv(c0, net.conv1[0], ctx.conv_out(net.conv1[0], c0.hw), LEAKY01), net.conv1_1[0], View(cat1, 0, 128), LEAKY01)
    c2 = conv(c1, net.conv2[0], ctx.conv_out(net.conv2[0], c1.hw), LEAKY01)
    c2 = conv(c2, net.conv2_1[0], ctx.conv_out(net.conv2_1[0], c2.hw), LEAKY01)
    flow2 = predict(c2, net.predict_flow2, n, H // 4, W // 4)
    flow_up(flow2, net.upsampled_flow2_to_1, View(cat1, 160, 2))
    conv(c2, net.deconv1[0], View(cat1, 128, 32), LEAKY01, transposed=True)
    i1 = conv(View(cat1, 0, 162), net.inter_conv1[0], ctx.conv_out(net.inter_conv1[0], (H // 2, W // 2)), 0)
    flow1 = predict(i1, net.predict_flow1, n, H // 2, W // 2)
    flow_up(flow1, net.upsampled_flow1_to_0, View(cat0, 80, 2))
    conv(View(cat1, 0, 162), net.deconv0[0], View(cat0, 64, 16), LEAKY01, transposed=True)
    i0 = conv(View(cat0, 0, 82), net.inter_conv0[0], ctx.conv_out(net.inter_conv0[0], (H, W)), 0)
    return predict(i0, net.predict_flow0, n, H, W)
