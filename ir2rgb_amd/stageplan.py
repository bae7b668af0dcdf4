"""The common convolution stage with its host work done once: ``ConvStageFn``'s straight-line case as a cached plan.

``autograd.ConvStageFn`` handles every stage of the networks (first layers over x-expanded images, padded widths, thin fp32
outputs, sample groups, evaluation-mode BatchNorm, backward flags ...) and pays for that generality in Python: ~30 us of
interpreter time per forward and ~40 us per backward on top of the launches, 226 times per training window -- a third of the
host time that bounds the loop once the GPU needs less than the host.  Nine stages in ten are
the same plain case -- conv -> training-mode BatchNorm -> activation (+ residuals) on a 64-multiple power-of-two width, as one
sample group or as the discriminators' batch of groups -- and everything about such a stage except its tensors is a
function of (module, input shape, spec): descriptors (forward, data gradient, weight gradient), output shapes, statistics rows, workspace sizes, the split of the
BatchNorm launches.  A ``StagePlan`` computes those once and then issues the SAME library calls with the SAME arguments as
the general path, in a handful of statements (``IR2RGB_LEAN_STAGE=0`` switches it off; tests/test_stage_backward_gpu.py
holds the two paths against each other bit for bit, forward and backward).

Anything else -- and any call while a side-stream weight gradient is on -- takes the general path.  The stream check
(ir2rgb_amd.streamcheck) runs the plans: they tag and check the same cached buffers as the general path -- packed weights and
the split-K workspace through the helpers both paths share, the BatchNorm running statistics and a gradient sink here.
"""
import os

import torch

from . import _lib
from . import conv as C
from . import layers as L
from . import streamcheck as SC

ENABLED = os.environ.get("IR2RGB_LEAN_STAGE", "1") != "0"
_F32 = torch.float32
_CL = torch.channels_last


class StagePlan:
    """One stage as ``groups`` >= 1 independent forwards batched along N (the discriminators' real | generated | raw
    frames): one convolution, BatchNorm per sample group by offset, and in backward the two things only the batched stages
    meet in production -- flags (autograd.backward_flags: no parameter gradients in the generator's pass) and passes in
    which only the leading k groups carry a gradient (the work then runs on that leading part of the batch; the rest of
    the gradient tensor stays unwritten, nobody reads it)."""
    __slots__ = ("desc", "out_shape", "stats_shape", "rows", "cout", "npix", "fused", "act", "dtc", "tdtype",
                 "ws_bytes", "nblk", "x_shape", "wdesc", "wshape", "wgrad_ws", "spec", "groups", "order", "dgrads")

    def __init__(self, x, spec, conv, bn, fused_bn):
        dt = spec["dtype"]
        cout = conv.out_channels
        self.spec = spec
        self.cout, self.tdtype, self.dtc = cout, dt, C._TORCH2DT[dt]
        self.x_shape = tuple(x.shape)
        G = self.groups = spec.get("groups", 1)
        self.order = tuple(spec.get("group_order") or range(G))
        d = self.desc = C.make_desc(self.x_shape, cout, spec["k"], spec["stride"], spec["pad"], spec["pad_mode"], dt,
                                    spec["transposed"], spec.get("output_padding", 0), act=0, out_f32=False,
                                    stats_per_sample=G > 1)
        if d.N % G:
            raise ValueError("conv stage: sample groups need N % groups == 0 and no residual inputs")
        self.out_shape = (d.N, d.Cout, d.Hout, d.Wout)
        self.rows = C.stats_rows(d)
        self.stats_shape = (self.rows, 2, cout)
        self.npix = d.N * d.Hout * d.Wout // G          # per sample group
        self.fused = bool(fused_bn and cout % 64 == 0 and self.rows // G <= L.FUSED_BN_MAX_ROWS)
        self.act = spec["act"]
        self.ws_bytes = C.fwd_workspace_bytes(d)
        self.nblk = _lib.query("ir2rgb_bn_bwd_blocks", self.npix, cout)
        self.dgrads = {}           # built at the first backward, per active batch size: dgrad_geometry + (workspace bytes,)
        self.wdesc = self.wshape = self.wgrad_ws = None

    # ------------------------------------------------------------------------------------------------------------
    def forward(self, ctx, x, bias, res1, res2, conv, bn):
        G = self.groups
        if G > 1 and (res1 is not None or res2 is not None):
            raise ValueError("conv stage: sample groups need N % groups == 0 and no residual inputs")
        if x.dtype is not self.tdtype or not x.is_contiguous(memory_format=_CL):
            raise ValueError("conv stage: x must be a channels_last half tensor of the stage's dtype")
        lib, d, dev, cout = _lib.lib(), self.desc, x.device, self.cout
        stream = _lib.current_stream(x)
        wp = L.packed_weight(conv, d, None, "w")
        y = torch.empty(self.out_shape, dtype=self.tdtype, device=dev, memory_format=_CL)
        stats = torch.empty(self.stats_shape, dtype=_F32, device=dev)
        ws, wsb = C._fwd_workspace(d, x) if self.ws_bytes else (None, 0)
        tok = C._prof_begin(d) if C.PROFILE is not None else None
        rc = lib.ir2rgb_conv2d_fwd_ws(d, x, wp, None, y, stats, ws, wsb, stream)
        if rc:
            _lib.check(rc, "conv2d_fwd")
        if tok is not None:
            C._prof_end(tok, d)
        # BatchNorm per group: [scale | shift | mean | invstd][group] in one allocation, everything addressed by offset
        # (no slices, no per-group wrappers)
        vec = torch.empty((4, G, cout), dtype=_F32, device=dev)
        z = torch.empty(self.out_shape, dtype=self.tdtype, device=dev, memory_format=_CL)
        _, pw, pb, prm, prv, has_rm, momentum, eps, trs = L._bn_ptrs(bn)
        track = trs and has_rm
        reps = L._STAT_UPDATES        # layers.repeated_forward: an int, or one count per group
        py, pz, ps, pv = y.data_ptr(), z.data_ptr(), stats.data_ptr(), vec.data_ptr()
        npix, rg, c4 = self.npix, self.rows // G, cout * 4
        per_y, per_s, gc4 = npix * cout * y.element_size(), rg * 2 * c4, G * c4
        for g in self.order:          # (the order the running statistics advance in)
            r = reps[g] if isinstance(reps, tuple) else reps
            sc = pv + g * c4
            if SC.ENABLED and track:      # the launch reads and advances them (as layers.bn_finalize / bn_finalize_apply)
                SC.consumed(bn.running_mean, "BatchNorm running statistics")
                SC.produced(bn.running_mean, "BatchNorm running statistics")
            if self.fused:
                rc = lib.ir2rgb_bn_finalize_apply(ps + g * per_s, rg, cout, npix, pw, pb, bias, prm if track else None,
                                                  prv if track else None, momentum, eps, sc, sc + gc4, sc + 2 * gc4, sc + 3 * gc4,
                                                  r, py + g * per_y, res1, res2, pz + g * per_y, npix, self.act, self.dtc, stream)
                if rc:
                    _lib.check(rc, "bn_finalize_apply")
            else:
                rc = lib.ir2rgb_bn_finalize_ex(ps + g * per_s, rg, cout, npix, pw, pb, bias, prm if track else None,
                                               prv if track else None, momentum, eps, sc, sc + gc4, sc + 2 * gc4, sc + 3 * gc4,
                                               r, 0, stream)
                if rc:
                    _lib.check(rc, "bn_finalize")
                rc = lib.ir2rgb_bn_apply(py + g * per_y, sc, sc + gc4, res1, res2, pz + g * per_y, npix, cout, self.act, self.dtc,
                                         stream)
                if rc:
                    _lib.check(rc, "bn_apply")
            if track and bn.num_batches_tracked is not None:
                L._PENDING_COUNTERS.append((bn.num_batches_tracked, r))
        ctx.plan = self
        ctx.conv = conv
        ctx.has_res = (res1 is not None, res2 is not None)
        ctx.save_for_backward(x, y, vec)
        return z

    # ------------------------------------------------------------------------------------------------------------
    def _build_wgrad(self, conv):
        spec = self.spec
        self.wdesc = d = C.make_desc(self.x_shape, self.cout, spec["k"], spec["stride"], spec["pad"], spec["pad_mode"], self.tdtype,
                                     bool(spec["transposed"]), spec.get("output_padding", 0))
        self.wshape = (d.Cin, d.Cout, d.kh, d.kw) if d.transposed else (d.Cout, d.Cin, d.kh, d.kw)
        self.wgrad_ws = (_lib.query("ir2rgb_conv2d_wgrad_workspace_elems", d),
                         _lib.query("ir2rgb_conv2d_wgrad_acc_workspace_elems", d))

    def backward(self, ctx, gz):
        A = _autograd()
        x, y, vec = ctx.saved_tensors
        conv = ctx.conv
        want_params = not (getattr(conv, "_ir2rgb_bwd", 0) & A.SKIP_PARAM_GRADS)
        G, ka = self.groups, getattr(conv, "_ir2rgb_active", None)
        if ka is None or ka >= G:
            ka = G
        elif want_params:
            raise RuntimeError("conv stage: a pass with inactive sample groups cannot produce parameter gradients")
        na = self.x_shape[0] // G * ka
        lib, dev, cout, dt = _lib.lib(), y.device, self.cout, self.tdtype
        stream = _lib.current_stream(y)
        if gz.dtype is not dt or not gz.is_contiguous(memory_format=_CL):
            gz = A._as_half_nhwc(gz, dt)
        # ---- BatchNorm + activation backward of the active groups: [dgamma | dbeta | partial rows] in one allocation (one
        # partial-row region serves all groups: same stream, one after the other)
        buf = torch.empty((self.nblk * 2 + 5) * cout, dtype=_F32, device=dev)
        gshape = (na,) + self.out_shape[1:]
        gy = torch.empty(gshape, dtype=dt, device=dev, memory_format=_CL)
        pv, pbuf, c4 = vec.data_ptr(), buf.data_ptr(), cout * 4
        gc4, npix = G * c4, self.npix
        per = npix * cout * y.element_size()
        pg, py, pgy = gz.data_ptr(), y.data_ptr(), gy.data_ptr()
        for g in range(ka):
            sc = pv + g * c4
            rc = lib.ir2rgb_bn_bwd(pg + g * per, py + g * per, sc, sc + gc4, sc + 2 * gc4, sc + 3 * gc4, pgy + g * per, pbuf,
                                   pbuf + c4, pbuf + 2 * c4, npix, cout, self.act | (32 if g else 0), self.dtc, stream)
            if rc:
                _lib.check(rc, "bn_bwd")
        need = ctx.needs_input_grad
        # ---- data gradient over the active samples, into a tensor of the full batch's shape
        dx = None
        if need[0]:
            dg = self.dgrads.get(na)
            if dg is None:
                dg = A.dgrad_geometry(self.spec, (na,) + self.x_shape[1:], gshape, dt)
                dg = self.dgrads[na] = dg + (C.fwd_workspace_bytes(dg[0]),)
            dd, dpack, adjoint, fold, nb = dg
            if fold:        # (reflection padding other than the in-place 3x3 adjoint: two launches, conv_dgrad's business)
                if ka == G:
                    dx = A.conv_dgrad(gy, conv, self.spec, self.x_shape)
                else:
                    dx = torch.empty(self.x_shape, dtype=dt, device=dev, memory_format=_CL)
                    A.conv_dgrad(gy, conv, self.spec, (na,) + self.x_shape[1:], out=dx[:na])
            else:
                wp = L.packed_weight(conv, dpack, None, "dgrad", adjoint)
                dx = torch.empty(self.x_shape, dtype=dt, device=dev, memory_format=_CL)
                ws, wsb = C._fwd_workspace(dd, gy) if nb else (None, 0)
                tok = C._prof_begin(dd) if C.PROFILE is not None else None
                rc = lib.ir2rgb_conv2d_fwd_ws(dd, gy, wp, None, dx, None, ws, wsb, stream)
                if rc:
                    _lib.check(rc, "conv2d_fwd")
                if tok is not None:
                    C._prof_end(tok, dd)
        hr = ctx.has_res
        r1, r2 = (gz if hr[0] else None), (gz if hr[1] else None)
        if not want_params:
            return dx, None, None, None, None, r1, r2, None, None, None
        # ---- weight gradient (whole batch: a pass that wants parameter gradients has every group active)
        dw = None
        if need[1]:
            if self.wdesc is None:
                self._build_wgrad(conv)
            wd = self.wdesc
            out, acc, dw = A.wgrad_destination(conv.weight, self.wshape)
            sink = out if dw is not None else None          # (the parameter's slice of a flat all-reduce buffer)
            if out is None:
                out = dw = torch.empty(self.wshape, dtype=_F32, device=dev)
            wsn = torch.empty(self.wgrad_ws[1 if acc else 0], dtype=_F32, device=dev)
            tok = C._prof_begin(wd, "wgrad") if C.PROFILE is not None else None
            rc = (lib.ir2rgb_conv2d_wgrad_acc if acc else lib.ir2rgb_conv2d_wgrad)(wd, x, gy, out, wsn, stream)
            if rc:
                _lib.check(rc, "conv2d_wgrad")
            if SC.ENABLED and sink is not None:
                SC.produced(sink, f"grad sink {self.wshape}")
            if tok is not None:
                C._prof_end(tok, wd, "conv_wgrad")
        # (training-mode BatchNorm removes the per-channel mean: the bias gradient is exactly zero = None)
        return dx, dw, None, buf[:cout], buf[cout:2 * cout], r1, r2, None, None, None


def _autograd():
    from . import autograd
    return autograd


def lookup(x, spec, conv, bn, fused_bn):
    """The plan of this stage call, or None when the general path has to run it."""
    if not ENABLED or bn is None or spec["first"] or not spec["training"]:
        return None
    A = _autograd()
    if A.WGRAD_SIDE_STREAM:
        return None
    plans = conv.__dict__.get("_ir2rgb_plans")
    if plans is None:
        plans = conv.__dict__["_ir2rgb_plans"] = {}
    key = (x.shape, spec["act"], spec["pad_mode"], spec["dtype"], spec["stride"], spec["pad"], spec["transposed"],
           spec["output_padding"], spec["out_f32"], spec["fused_leaky"], spec["fused_relu"], fused_bn, id(bn), spec["groups"],
           spec["group_order"])
    plan = plans.get(key)
    if plan is None:
        cout, cin = conv.out_channels, conv.in_channels
        ok = (not spec["out_f32"] and not spec["fused_leaky"] and not spec["fused_relu"] and A.padded_width(cout) == cout
              and A.padded_width(cin) == cin and x.dim() == 4 and x.shape[1] == cin and x.is_cuda
              and isinstance(bn, torch.nn.Module))
        if ok and spec["groups"] > 1:
            ok = x.shape[0] % spec["groups"] == 0
        plan = plans[key] = StagePlan(x, spec, conv, bn, fused_bn) if ok else False
        if len(plans) > 64:
            plans.clear()
    return plan or None
