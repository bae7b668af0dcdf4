"""fp64 replays of the non-convolution entry points (test-only): heads, warp blend, FlowNet2 glue and operators (cost
volume, pixel-space warp, channel norm, with their gradients), pooling, layout helpers, grouped losses, Adam.

REPLAY maps an entry point to ``replay_*(dev, rec, g)``: ``rec`` a ``"kind": "op"`` record in the format of
tests/window_geometries.json, ``g`` its generator (oracle.replay.gen).  References are oracle/window_ops_ref.py's and
oracle/flow_ops_ref.py's, bounds oracle/bounds.py's, fixed before anything runs.  Entries that take a dtype run in bf16 and f16 from one fp64 reference
on operands exact in both formats.  Every element is compared, and what a launch must leave alone is checked too:
channels outside a slice, dT channels >= Cout*KH (zero), loss slots no term names, the pool bytes around each Adam
tensor.  Bias gradients and loss slots must repeat bit for bit.  Each replay returns {format: worst err/bound}.
tests/test_window_ops_gpu.py runs them at the window's records, tests/test_edge_ops_gpu.py at oracle/edge_records.py's.
"""
import numpy as np
import torch

from oracle import bounds as B
from oracle import conv_ref as R
from oracle import flow_ops_ref as F
from oracle import window_ops_ref as O
from oracle.replay import DTYPES, assert_bound, bits, call, exact, hand, np64, sentinel

ARGS = {    # argument names of the header's prototypes, without the stream
    "ir2rgb_gather_f32": "src idx dst n",
    "ir2rgb_avgpool3s2": "x y planes H W backward",
    "ir2rgb_xexpand": "inp out N Cin H W Wout KW stride_w pad_w pad_mode dtype",
    "ir2rgb_xexpand_cx": "inp out N Cin H W Wout KW stride_w pad_w pad_mode Cx dtype",
    "ir2rgb_flow_upsample_slice": "inp weight bias out N h w ld c_off dtype",
    "ir2rgb_nchw_f32_to_nhwc_half": "inp out N C H W dtype",
    "ir2rgb_nhwc_half_to_nchw_f32": "inp out N C H W dtype",
    "ir2rgb_nchw_f32_to_nhwc_half_slice": "inp out N C H W ld c_off act dtype",
    "ir2rgb_head_finish": "T bias out N H W Cout KH CT pad_h acts mul",
    "ir2rgb_warp_blend_fwd": "raw prev flow w out warp_out N Cp H W",
    "ir2rgb_thin_grad_expand": "gz g64 g8 dbias N Cout H W dtype",
    "ir2rgb_fold_reflect": "dxpad dx N H W C pad_h pad_w dtype",
    "ir2rgb_head_finish_bwd": "gout out dT dbias partial N H W Cout KH CT pad_h acts mul dtype",
    "ir2rgb_warp_blend_bwd": "gout raw prev flow w graw gflow gw N Cp H W",
    "ir2rgb_xexpand_bwd": "dxe din N Cin H W Wout KW stride_w pad_w pad_mode dtype",
    "ir2rgb_warp_diff_norm_fwd": "img1 img2 flow warped diff norm N C H W",
    "ir2rgb_channelnorm_fwd": "inp out N C H W norm_deg",
    "ir2rgb_correlation_fwd": "in1 in2 out N C H W pad_size kernel_size max_displacement stride1 stride2",
    "ir2rgb_correlation_bwd": "in1 in2 gout gin1 gin2 N C H W pad_size kernel_size max_displacement stride1 stride2",
    "ir2rgb_correlation_nhwc_half": "a lda offa b ldb offb out out_mode ldo offo slope N C H W dtype",
    "ir2rgb_resample2d_fwd": "img flow out N C H W kernel_size",
    "ir2rgb_resample2d_bwd": "img flow gout gimg gflow N C H W kernel_size",
    "ir2rgb_channelnorm_bwd": "inp out gout gin N C H W norm_deg",
}


def named_args(rec):
    return dict(zip(ARGS[rec["entry"]].split(), rec["args"]))


def _ranged(dev, rec, mode):
    """``mode`` of a replay: the inputs of oracle/range_cases.py (overflow / subnormal / nonfinite) under
    oracle.bounds.check_range, at an EDGE_RANGE record."""
    from oracle import range_cases as RC
    return RC.run(dev, rec, mode, RC.build_for(rec))


# ---------------------------------------------------------------------------------------------------------------------
def replay_gather(dev, rec, g):
    a = named_args(rec)
    n = a["n"]
    src = torch.randn(n, generator=g)
    idx = torch.randint(-1, n, (n,), generator=g, dtype=torch.int32)
    dst = sentinel((n,), torch.float32, dev)
    call(rec["entry"], src.to(dev), idx.to(dev), dst, n)
    torch.cuda.synchronize()
    ref = torch.where(idx >= 0, src[idx.clamp(min=0).long()], torch.zeros(()))
    return {"f32": exact("gather", dst, ref.double())}


def replay_avgpool(dev, rec, g):
    a = named_args(rec)
    P, H, W = a["planes"], a["H"], a["W"]
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if not a["backward"]:
        x = R.draw((P, H, W), g)
        y = sentinel((P, Ho, Wo), torch.float32, dev)
        call(rec["entry"], x.to(dev), y, P, H, W, 0)
        torch.cuda.synchronize()
        ref, S = O.avgpool3s2(np64(x))
        terms = 10          # <= 9 taps and the division
    else:
        gy = R.draw((P, Ho, Wo), g)
        y = sentinel((P, H, W), torch.float32, dev)
        call(rec["entry"], gy.to(dev), y, P, H, W, 1)
        torch.cuda.synchronize()
        ref, S = O.avgpool3s2_bwd(np64(gy), H, W)
        terms = 8           # <= 4 quotients (one rounding each) and their sum
    return {"f32": assert_bound("avgpool3s2", *B.check_bound(np64(y), ref, B.bound_sum(ref, S, "f32", terms)), ref.shape)}


def replay_xexpand(dev, rec, g, mode=None):
    if mode is not None:
        return _ranged(dev, rec, mode)
    a = named_args(rec)
    N, Cin, H, W, Wout, KW, s, p, pm = (a[k] for k in "N Cin H W Wout KW stride_w pad_w pad_mode".split())
    Cx = a.get("Cx", 64)
    x = torch.randn(N, Cin, H, W, generator=g)
    ref = O.xexpand(np64(x), Wout, KW, s, p, pm, Cx)
    out = {}
    for fmt, dtype, dt in DTYPES:
        y = sentinel((N, H, Wout, Cx), dtype, dev)
        args = (N, Cin, H, W, Wout, KW, s, p, pm) + ((Cx,) if "Cx" in a else ()) + (dt,)
        call(rec["entry"], x.to(dev), y, *args)
        torch.cuda.synchronize()
        out[fmt] = exact(f"{fmt} xexpand", y, torch.from_numpy(ref))
    return out


def replay_xexpand_bwd(dev, rec, g, mode=None):
    if mode is not None:
        return _ranged(dev, rec, mode)
    a = named_args(rec)
    N, Cin, H, W, Wout, KW, s, p, pm = (a[k] for k in "N Cin H W Wout KW stride_w pad_w pad_mode".split())
    dxe = R.draw((N, H, Wout, 64), g)
    ref, cnt = O.xexpand_bwd(np64(dxe), Cin, W, KW, s, p, pm)
    S, _ = O.xexpand_bwd(np.abs(np64(dxe)), Cin, W, KW, s, p, pm)
    out = {}
    for fmt, dtype, dt in DTYPES:
        din = sentinel((N, Cin, H, W), torch.float32, dev)
        call(rec["entry"], dxe.to(dev, dtype), din, N, Cin, H, W, Wout, KW, s, p, pm, dt)
        torch.cuda.synchronize()
        bnd = B.bound_sum(ref, S, "f32", int(cnt.max()))
        out[fmt] = assert_bound(f"{fmt} xexpand_bwd", *B.check_bound(np64(hand("out", f"{fmt} din", din)), ref, bnd), ref.shape)
    return out


def replay_fold(dev, rec, g, mode=None):
    if mode is not None:
        return _ranged(dev, rec, mode)
    a = named_args(rec)
    N, H, W, C, ph, pw = (a[k] for k in "N H W C pad_h pad_w".split())
    dxpad = R.draw((N, H + 2 * ph, W + 2 * pw, C), g)
    ref, cnt = O.fold_reflect(np64(dxpad), ph, pw)
    S, _ = O.fold_reflect(np.abs(np64(dxpad)), ph, pw)
    out = {}
    for fmt, dtype, dt in DTYPES:
        dx = sentinel((N, H, W, C), dtype, dev)
        call(rec["entry"], dxpad.to(dev, dtype), dx, N, H, W, C, ph, pw, dt)
        torch.cuda.synchronize()
        bnd = B.bound_sum(ref, S, fmt, int(cnt.max()))
        out[fmt] = assert_bound(f"{fmt} fold_reflect", *B.check_bound(np64(hand("out", f"{fmt} dx", dx)), ref, bnd), ref.shape)
    return out


def replay_thin_grad(dev, rec, g, mode=None):
    if mode is not None:
        return _ranged(dev, rec, mode)
    a = named_args(rec)
    N, Cout, H, W = a["N"], a["Cout"], a["H"], a["W"]
    gz = torch.randn(N, Cout, H, W, generator=g)
    npix = N * H * W
    want = torch.zeros(N, H, W, 8, dtype=torch.float64)
    want[..., :Cout] = gz.double().permute(0, 2, 3, 1)
    chain = -(-npix // 256) + 8         # a thread's pixels, then the 256-lane tree
    ref = gz.double().sum((0, 2, 3)).numpy()
    S = gz.double().abs().sum((0, 2, 3)).numpy()
    out = {}
    for fmt, dtype, dt in DTYPES:
        runs = []
        for _ in range(2):
            g64 = sentinel((N, H, W, 64), dtype, dev)
            g8 = sentinel((N, H, W, 8), dtype, dev)
            db = sentinel((Cout,), torch.float32, dev)
            call(rec["entry"], gz.to(dev), g64, g8, db, N, Cout, H, W, dt)
            torch.cuda.synchronize()
            runs.append(db.cpu())
        exact(f"{fmt} g8", g8, want)
        exact(f"{fmt} g64 (channels < 8)", g64[..., :8], want)
        assert not bool(g64[..., 8:].ne(0).any()), f"{fmt}: g64 channels >= 8 are not zero"
        assert torch.equal(bits(runs[0]), bits(runs[1])), f"{fmt}: dbias differs between two runs"
        out[fmt] = assert_bound(f"{fmt} dbias", *B.check_bound(np64(hand("out", f"{fmt} dbias", runs[0])), ref,
                                                                B.bound_rw(ref, S, "f32", chain, 0)), ref.shape)
    return out


def replay_flow_up(dev, rec, g, mode=None):
    if mode is not None:
        return _ranged(dev, rec, mode)
    a = named_args(rec)
    N, h, w, ld, off = a["N"], a["h"], a["w"], a["ld"], a["c_off"]
    x = R.draw((N, 2, h, w), g, 4.0)
    wt = R.draw((2, 2, 4, 4), g, 0.5)
    bias = R.draw((2,), g) if a["bias"] else None
    ref, S = O.flow_upsample(np64(x), np64(wt), None if bias is None else np64(bias))
    ref, S = ref.transpose(0, 2, 3, 1), S.transpose(0, 2, 3, 1)
    out = {}
    for fmt, dtype, dt in DTYPES:
        buf = R.draw((N, 2 * h, 2 * w, ld), g).to(dev, dtype)
        before = buf.clone()
        call(rec["entry"], x.to(dev), wt.to(dev), None if bias is None else bias.to(dev), buf, N, h, w, ld, off, dt)
        torch.cuda.synchronize()
        keep = torch.ones(ld, dtype=torch.bool)
        keep[off:off + 2] = False
        assert torch.equal(buf[..., keep], before[..., keep]), f"{fmt}: flow up-sampler wrote outside its channels"
        got = np64(buf[..., off:off + 2])
        out[fmt] = assert_bound(f"{fmt} flow_upsample", *B.check_bound(got, ref, B.bound_sum(ref, S, fmt, 9)), ref.shape)
    return out


def launch_convert(dev, rec, x, fmt):
    """One launch of a layout converter on x [N,C,H,W] fp32 (for ir2rgb_nhwc_half_to_nchw_f32: the values of its half
    input).  -> the output as an fp64 array in the reference's layout; the slice form asserts its neighbours untouched."""
    a = named_args(rec)
    N, C, H, W = a["N"], a["C"], a["H"], a["W"]
    dtype, dt = {f: (t, d) for f, t, d in DTYPES}[fmt]
    entry = rec["entry"]
    if entry == "ir2rgb_nhwc_half_to_nchw_f32":
        y = sentinel((N, C, H, W), torch.float32, dev)
        call(entry, x.permute(0, 2, 3, 1).contiguous().to(dev, dtype), y, N, C, H, W, dt)
        torch.cuda.synchronize()
        return np64(y)
    if entry == "ir2rgb_nchw_f32_to_nhwc_half":
        y = sentinel((N, H, W, C), dtype, dev)
        call(entry, x.contiguous().to(dev), y, N, C, H, W, dt)
        torch.cuda.synchronize()
        return np64(y)
    ld, off = a["ld"], a["c_off"]
    buf = torch.randn(N, H, W, ld, generator=torch.Generator().manual_seed(ld)).to(dev, dtype)
    before = buf.clone()
    call(entry, x.contiguous().to(dev), buf, N, C, H, W, ld, off, a["act"], dt)
    torch.cuda.synchronize()
    keep = torch.ones(ld, dtype=torch.bool)
    keep[off:off + C] = False
    assert torch.equal(bits(buf[..., keep]), bits(before[..., keep])), f"{fmt}: the converter wrote outside its channels"
    return np64(buf[..., off:off + C])


def replay_convert(dev, rec, g, mode=None):
    """The layout converters: every element bit for bit the fp64 value rounded to nearest even into the output format.
    ``mode``: the inputs of oracle/range_cases.py (beyond f16's range, subnormal, inf / NaN) under the same comparison."""
    if mode is not None:
        return _ranged(dev, rec, mode)
    a = named_args(rec)
    x = torch.randn(a["N"], a["C"], a["H"], a["W"], generator=g)
    out = {}
    for fmt, dtype, _ in DTYPES:
        if rec["entry"] == "ir2rgb_nhwc_half_to_nchw_f32":
            xin = x.to(dtype).float()
            ref, want_dt = xin.double(), torch.float32
        else:
            xin = x
            ref, want_dt = torch.from_numpy(O.nchw_to_nhwc(np64(x), a.get("act", 0))), dtype
        got = torch.from_numpy(launch_convert(dev, rec, xin, fmt)).to(want_dt)
        out[fmt] = exact(f"{fmt} {rec['entry']}", got, ref)
    return out


def replay_head_finish(dev, rec, g):
    a = named_args(rec)
    N, H, W, Cout, KH, CT, pad, acts, mul = (a[k] for k in "N H W Cout KH CT pad_h acts mul".split())
    T = R.draw((N, H, W, CT), g, 0.5)
    bias = R.draw((Cout,), g, 0.5) if a["bias"] else None
    ref, _, S = O.head_finish(np64(T), None if bias is None else np64(bias), Cout, KH, pad, acts, mul)
    y = sentinel((N, Cout, H, W), torch.float32, dev)
    call(rec["entry"], T.to(dev), None if bias is None else bias.to(dev), y, N, H, W, Cout, KH, CT, pad, acts, mul)
    torch.cuda.synchronize()
    bnd = B.bound_act(ref, O.act_slope(ref, acts, mul, Cout), S, KH + 1)
    return {"f32": assert_bound("head_finish", *B.check_bound(np64(y), ref, bnd), ref.shape)}


def replay_head_finish_bwd(dev, rec, g, mode=None):
    if mode is not None:
        return _ranged(dev, rec, mode)
    from ir2rgb_amd import _lib
    a = named_args(rec)
    N, H, W, Cout, KH, CT, pad, acts, mul = (a[k] for k in "N H W Cout KH CT pad_h acts mul".split())
    pre = torch.randn(N, Cout, H, W, generator=g, dtype=torch.float64) * 2
    o64 = np.empty(pre.shape)
    for co in range(Cout):
        nb = O.nibble(acts, co)
        p = pre[:, co].numpy()
        o64[:, co] = np.tanh(p) if nb == 1 else (1 / (1 + np.exp(-p)) if nb == 2 else p * mul)
    outv = torch.from_numpy(o64).float()
    gout = torch.randn(N, Cout, H, W, generator=g)
    ref, dbias, S, Sb = O.head_finish_bwd(np64(gout), np64(outv), Cout, KH, CT, pad, acts, mul)
    rows = _lib.lib().ir2rgb_head_finish_bwd_rows(N, H, W)
    chain = -(-N * H * W // (rows * 256)) + 256 + -(-rows // 32) + 32
    out = {}
    for fmt, dtype, dt in DTYPES:
        runs = []
        for _ in range(2):
            dT = sentinel((N, H, W, CT), dtype, dev)
            db = sentinel((Cout,), torch.float32, dev)
            part = torch.empty(rows * 8, dtype=torch.float32, device=dev)
            call(rec["entry"], gout.to(dev), outv.to(dev), dT, db, part, N, H, W, Cout, KH, CT, pad, acts, mul, dt)
            torch.cuda.synchronize()
            runs.append(db.cpu())
        assert torch.equal(bits(runs[0]), bits(runs[1])), f"{fmt}: dbias differs between two runs"
        assert not bool(dT[..., Cout * KH:].ne(0).any()), f"{fmt}: dT channels >= Cout*KH are not zero"
        r1 = assert_bound(f"{fmt} dT", *B.check_bound(np64(dT), ref, B.bound_rw(ref, S, fmt, 3, 6)), ref.shape)
        r2 = assert_bound(f"{fmt} dbias", *B.check_bound(np64(runs[0]), dbias, B.bound_rw(dbias, Sb, "f32", chain, 6)),
                     dbias.shape)
        out[fmt] = max(r1, r2)
    return out


# warp_blend: flows drawn so that the fp64 sampling coordinates lie >= 0.02 from a cell edge, plus a band of pixels
# (about 3 %) that sample beyond the border, where the clamp is active and the flow gradient must be zero
def _warp_inputs(N, Cp, H, W, g):
    def flow_1d(n, shape):
        base = torch.arange(n, dtype=torch.float64).view([1] * (len(shape) - 1) + [n]).expand(shape)
        cell = (base + torch.randint(-6, 7, shape, generator=g)).clamp(0, n - 2)
        t = cell + 0.02 + 0.96 * torch.rand(shape, generator=g, dtype=torch.float64)
        out_band = torch.rand(shape, generator=g) < 0.03
        beyond = torch.where(torch.rand(shape, generator=g) < 0.5, -0.05 - 2 * torch.rand(shape, generator=g, dtype=torch.float64),
                             n - 1 + 0.05 + 2 * torch.rand(shape, generator=g, dtype=torch.float64))
        t = torch.where(out_band, beyond, t)
        return ((t + 0.5) * (n - 1) / n - base).float()
    fx = flow_1d(W, (N, H, W))
    fy = flow_1d(H, (N, W, H)).transpose(1, 2)
    flow = torch.stack([fx, fy], 1).contiguous()
    raw = R.draw((N, 3, H, W), g)
    prev = R.draw((N, Cp, H, W), g)
    w = torch.rand(N, 1, H, W, generator=g).to(torch.bfloat16).float()
    return raw, prev, flow, w


def _ambiguous(r, H, W):
    dx, dy = B.coord_delta(W), B.coord_delta(H)
    ix, iy = r["ix"], r["iy"]
    ax = (np.abs(ix - np.round(ix)) <= dx)
    ay = (np.abs(iy - np.round(iy)) <= dy)
    return ax | ay


def replay_warp_fwd(dev, rec, g):
    a = named_args(rec)
    N, Cp, H, W = a["N"], a["Cp"], a["H"], a["W"]
    raw, prev, flow, w = _warp_inputs(N, Cp, H, W, g)
    r = O.warp_blend(np64(raw), np64(prev), np64(flow), np64(w))
    dx, dy = B.coord_delta(W), B.coord_delta(H)
    y = sentinel((N, 3, H, W), torch.float32, dev)
    wo = sentinel((N, 3, H, W), torch.float32, dev) if a["warp_out"] else None
    call(rec["entry"], raw.to(dev), prev.to(dev), flow.to(dev), w.to(dev), y, wo, N, Cp, H, W)
    torch.cuda.synchronize()
    bnd = B.C_AR * B.U32 * r["S_out"] + r["dout_dix"][:, :] * dx + r["dout_diy"] * dy + B.ETA["f32"]
    ratio = assert_bound("warp_blend out", *B.check_bound(np64(y), r["out"], bnd), bnd.shape)
    if wo is not None:
        bw = B.C_AR * B.U32 * r["S_warp"] + r["dwarp_dix"] * dx + r["dwarp_diy"] * dy + B.ETA["f32"]
        ratio = max(ratio, assert_bound("warp_blend warp", *B.check_bound(np64(wo), r["warp"], bw), bw.shape))
    return {"f32": ratio}


def replay_warp_bwd(dev, rec, g):
    a = named_args(rec)
    N, Cp, H, W = a["N"], a["Cp"], a["H"], a["W"]
    raw, prev, flow, w = _warp_inputs(N, Cp, H, W, g)
    gout = R.draw((N, 3, H, W), g)
    args = [np64(t) for t in (raw, prev, flow, w)]
    r = O.warp_blend(*args, gout=np64(gout))
    dx, dy = B.coord_delta(W), B.coord_delta(H)
    graw = sentinel((N, 3, H, W), torch.float32, dev)
    gflow = sentinel((N, 2, H, W), torch.float32, dev)
    gw = sentinel((N, 1, H, W), torch.float32, dev)
    call(rec["entry"], gout.to(dev), raw.to(dev), prev.to(dev), flow.to(dev), w.to(dev), graw, gflow, gw, N, Cp, H, W)
    torch.cuda.synchronize()
    r1 = assert_bound("graw", *B.check_bound(np64(graw), r["graw"], B.U32 * np.abs(r["graw"]) + B.ETA["f32"]), r["graw"].shape)
    bgw = B.C_AR * B.U32 * r["S_gw"] + r["dgw_dix"] * dx + r["dgw_diy"] * dy + B.ETA["f32"]
    r2 = assert_bound("gw", *B.check_bound(np64(gw), r["gw"], bgw), bgw.shape)
    bgf = B.C_AR * B.U32 * r["S_gflow"] + np.stack([r["dgflow_x_diy"] * dy, r["dgflow_y_dix"] * dx], 1) + B.ETA["f32"]
    got = np64(gflow)
    amb = np.broadcast_to(_ambiguous(r, H, W)[:, None], got.shape)
    err = np.abs(got - r["gflow"])
    if amb.any():       # one-sided values: the cell on either side of the edge, the clamp on or off
        for kw in ({"keep_clamped_grad": True},):
            alt = O.warp_blend(*args, gout=np64(gout), **kw)["gflow"]
            err = np.where(amb, np.minimum(err, np.abs(got - alt)), err)
        for sx_, sy_ in ((-1, 0), (1, 0), (0, -1), (0, 1)):
            f2 = args[2].copy()
            f2[:, 0] += 2 * sx_ * dx
            f2[:, 1] += 2 * sy_ * dy
            alt = O.warp_blend(args[0], args[1], f2, args[3], gout=np64(gout))["gflow"]
            err = np.where(amb, np.minimum(err, np.abs(got - alt)), err)
    ratio = err / bgf
    i = int(np.argmax(ratio))
    assert np.isfinite(got).all() and ratio.max() <= 1.0, \
        f"gflow: {int((ratio > 1).sum())} elements over the bound (worst {ratio.max():.3g} at {np.unravel_index(i, got.shape)})"
    clamped = ~((r["ix"] > 0) & (r["ix"] < W - 1))
    assert clamped.sum() > 0 and not np.any(got[:, 0][clamped & ~amb[:, 0]]), "flow gradient not zero where clamped"
    print(f"\n  warp_blend_bwd: {int(amb[:, 0].sum())} pixels in the ambiguity band, {int(clamped.sum())} clamped in x")
    return {"f32": max(r1, r2, float(ratio.max()))}


# FlowNet2's fused warp -> diff -> channel norm: pixel-space flows drawn >= 0.02 from a cell edge (xf = x + dx is one
# fp32 rounding, far inside coord_delta), some beyond the border (corners clamped)
def _pixel_flow(N, H, W, g):
    def comp(n, shape):
        base = torch.arange(n, dtype=torch.float64).view([1] * (len(shape) - 1) + [n]).expand(shape)
        cell = base + torch.randint(-8, 9, shape, generator=g)
        t = cell + 0.02 + 0.96 * torch.rand(shape, generator=g, dtype=torch.float64)
        return (t - base).float()
    return torch.stack([comp(W, (N, H, W)), comp(H, (N, W, H)).transpose(1, 2)], 1).contiguous()


def replay_warp_diff_norm(dev, rec, g):
    a = named_args(rec)
    N, C, H, W = a["N"], a["C"], a["H"], a["W"]
    img1, img2 = R.draw((N, C, H, W), g), R.draw((N, C, H, W), g)
    flow = _pixel_flow(N, H, W, g)
    v, dvx, dvy, S = O.resample2d(np64(img2), np64(flow))
    d = np64(img1) - v
    ev = B.C_AR * B.U32 * S + dvx * B.coord_delta(W) + dvy * B.coord_delta(H)
    ed = ev + B.U32 * (np.abs(d) + np.abs(np64(img1)))
    outs = {k: (sentinel((N, C, H, W), torch.float32, dev) if a[k] else None) for k in ("warped", "diff")}
    norm = sentinel((N, 1, H, W), torch.float32, dev) if a["norm"] else None
    call(rec["entry"], img1.to(dev), img2.to(dev), flow.to(dev), outs["warped"], outs["diff"], norm, N, C, H, W)
    torch.cuda.synchronize()
    ratio = 0.0
    if outs["warped"] is not None:
        ratio = assert_bound("warped", *B.check_bound(np64(outs["warped"]), v, ev + B.ETA["f32"]), v.shape)
    if outs["diff"] is not None:
        ratio = max(ratio, assert_bound("diff", *B.check_bound(np64(outs["diff"]), d, ed + B.ETA["f32"]), d.shape))
    if norm is not None:
        # |d norm| <= sum_c |d_c| / norm * e_c <= sum_c e_c, and the squares, sum and sqrt: (C + 2) roundings of norm
        nr = np.sqrt((d * d).sum(1, keepdims=True))
        bn = ed.sum(1, keepdims=True) + (C + 2) * B.U32 * nr + B.ETA["f32"]
        ratio = max(ratio, assert_bound("norm", *B.check_bound(np64(norm), nr, bn), nr.shape))
    return {"f32": ratio}


def replay_channelnorm(dev, rec, g):
    a = named_args(rec)
    N, C, H, W = a["N"], a["C"], a["H"], a["W"]
    x = torch.randn(N, C, H, W, generator=g)
    ref = np.sqrt((np64(x) ** 2).sum(1, keepdims=True))
    y = sentinel((N, 1, H, W), torch.float32, dev)
    call(rec["entry"], x.to(dev), y, N, C, H, W, a["norm_deg"])
    torch.cuda.synchronize()
    bnd = (C + 2) * B.U32 * ref + B.ETA["f32"]
    return {"f32": assert_bound("channelnorm", *B.check_bound(np64(y), ref, bnd), ref.shape)}


# ---------------------------------------------------------------------------------------------------------------------
# FlowNet2 operators (references: oracle/flow_ops_ref.py).  Record keys beside the arguments: ``offset`` {tensor name:
# elements} moves a tensor's base pointer off its allocation's alignment; ``far`` [fx, fy] is added to every flow vector
# (all pixels sample beyond one border); ``scale`` multiplies the channel norm's input; ``modes`` lists the out modes of
# the half-precision cost volume to run (default: the recorded one).
def _at(t, rec, name, dev):
    """``t`` on the device, its first element ``rec["offset"][name]`` elements into a fresh allocation."""
    off = rec.get("offset", {}).get(name, 0)
    buf = torch.empty(t.numel() + off, dtype=t.dtype, device=dev)
    v = buf[off:].view(t.shape)
    v.copy_(t)
    return v


def _twice(name, launch, outs):
    """launch() -> tuple of output tensors, run twice into re-filled buffers: the named outputs must repeat bit for bit."""
    first = launch()
    torch.cuda.synchronize()
    again = launch()
    torch.cuda.synchronize()
    for k, a, b in zip(outs, first, again):
        if k is not None:
            assert torch.equal(bits(a.contiguous()), bits(b.contiguous())), f"{name}: {k} differs between two runs"
    return first


def corr_geometry(a):
    return tuple(a[k] for k in "pad_size kernel_size max_displacement stride1 stride2".split())


def replay_corr_fwd(dev, rec, g):
    from oracle.edge_records import corr_form
    a = named_args(rec)
    N, C, H, W = a["N"], a["C"], a["H"], a["W"]
    pad, k, md, s1, s2 = corr_geometry(a)
    f1, f2 = torch.randn(N, C, H, W, generator=g), torch.randn(N, C, H, W, generator=g)
    ref, S = F.correlation(np64(f1), np64(f2), pad, k, md, s1, s2)
    d1, d2 = _at(f1, rec, "in1", dev), f2.to(dev)

    def launch():
        out = _at(torch.full(ref.shape, float("nan")), rec, "out", dev)
        call(rec["entry"], d1, d2, out, N, C, H, W, pad, k, md, s1, s2)
        return (out,)
    out, = _twice("correlation_fwd", launch, ("out",))
    form = corr_form(N, C, H, W, pad, k, md, s1, s2, not rec.get("offset")).split(":")[0]
    bnd = B.bound_sum(ref, S, "f32", k * k * C + 2)
    return {form: assert_bound(f"correlation_fwd ({form})", *B.check_bound(np64(out), ref, bnd), ref.shape)}


def replay_corr_bwd(dev, rec, g):
    a = named_args(rec)
    N, C, H, W = a["N"], a["C"], a["H"], a["W"]
    pad, k, md, s1, s2 = corr_geometry(a)
    oc, oh, ow = F.correlation_out_shape(H, W, pad, k, md, s1, s2)
    f1, f2 = torch.randn(N, C, H, W, generator=g), torch.randn(N, C, H, W, generator=g)
    gout = torch.randn(N, oc, oh, ow, generator=g)
    r1, r2, S1, S2, L1, L2 = F.correlation_bwd(np64(f1), np64(f2), np64(gout), pad, k, md, s2)
    d1, d2, dg = f1.to(dev), f2.to(dev), gout.to(dev)

    def launch():
        g1, g2 = sentinel(f1.shape, torch.float32, dev), sentinel(f1.shape, torch.float32, dev)
        call(rec["entry"], d1, d2, dg, g1, g2, N, C, H, W, pad, k, md, s1, s2)
        return g1, g2
    g1, g2 = _twice("correlation_bwd", launch, ("gin1", "gin2"))
    ra = assert_bound("gin1", *B.check_bound(np64(g1), r1, B.bound_sum(r1, S1, "f32", L1 + 2)), r1.shape)
    rb = assert_bound("gin2", *B.check_bound(np64(g2), r2, B.bound_sum(r2, S2, "f32", L2 + 2)), r2.shape)
    return {"f32": max(ra, rb)}


def leaky(x, slope):
    return np.where(x > 0, x, x * slope)


def replay_corr_mfma(dev, rec, g, mode=None):
    if mode is not None:
        return _ranged(dev, rec, mode)
    a = named_args(rec)
    N, C, H, W = a["N"], a["C"], a["H"], a["W"]
    lda, offa, ldb, offb, ldo, offo, slope = (a[k] for k in "lda offa ldb offb ldo offo slope".split())
    f1, f2 = R.draw((N, C, H, W), g), R.draw((N, C, H, W), g)
    ref, S = F.correlation(np64(f1), np64(f2), 20, 1, 20, 1, 2)
    out = {}
    for fmt, dtype, dt in DTYPES:
        bufs = []
        for f, ld, off in ((f1, lda, offa), (f2, ldb, offb)):       # NaN in every channel outside the slice
            t = torch.full((N, H, W, ld), float("nan"), dtype=dtype)
            t[..., off:off + C] = f.permute(0, 2, 3, 1).to(dtype)
            bufs.append(t.to(dev))
        before = [t.clone() for t in bufs]
        for mode in rec.get("modes", [a["out_mode"]]):
            def launch():
                o = sentinel((N, 441, H, W), torch.float32, dev) if mode == 0 else \
                    sentinel((N, H, W, ldo), dtype, dev)
                call(rec["entry"], bufs[0], lda, offa, bufs[1], ldb, offb, o, mode, ldo, offo, slope, N, C, H, W, dt)
                return (o,)
            o, = _twice(f"{fmt} out_mode {mode}", launch, ("out",))
            if mode == 0:
                got, want, ofmt = np64(o), ref, "f32"
            else:
                keep = torch.ones(ldo, dtype=torch.bool)
                keep[offo:offo + 441] = False
                assert bool(torch.isnan(o[..., keep]).all()), f"{fmt}: the cost volume wrote outside its channels"
                got, want, ofmt = np64(o[..., offo:offo + 441].permute(0, 3, 1, 2)), leaky(ref, slope), fmt
            out[f"{fmt}/out{mode}"] = assert_bound(f"{fmt} out_mode {mode}", *B.check_bound(got, want, B.bound(want, S, ofmt, C + 2)),
                                                   want.shape)
        for t, b0 in zip(bufs, before):
            assert torch.equal(bits(t), bits(b0)), f"{fmt}: an input buffer was written"
    return out


def _resample_inputs(rec, g):
    a = named_args(rec)
    N, C, H, W = a["N"], a["C"], a["H"], a["W"]
    img = torch.randn(N, C, H, W, generator=g)
    flow = _pixel_flow(N, H, W, g)
    if "far" in rec:
        flow = (flow + torch.tensor(rec["far"], dtype=torch.float32).view(1, 2, 1, 1)).contiguous()
    return a, img, flow


def replay_resample_fwd(dev, rec, g):
    a, img, flow = _resample_inputs(rec, g)
    N, C, H, W = img.shape
    v, dvx, dvy, S = F.resample2d(np64(img), np64(flow))
    ev = B.C_AR * B.U32 * S + dvx * B.coord_delta(W) + dvy * B.coord_delta(H)
    di, df = img.to(dev), flow.to(dev)

    def launch():
        out = sentinel(img.shape, torch.float32, dev)
        call(rec["entry"], di, df, out, N, C, H, W, a["kernel_size"])
        return (out,)
    out, = _twice("resample2d_fwd", launch, ("out",))
    return {"f32": assert_bound("warped", *B.check_bound(np64(out), v, ev + B.ETA["f32"]), v.shape)}


def resample_bwd_bounds(r, C, H, W):
    """(gimg bound, gflow bound) of a flow_ops_ref.resample2d_bwd result: L contributions of up to three roundings each
    (the two weight products, times gout) and their additions in any order; 8 products per channel (4 per component, two
    roundings each) in a chain of 4 C, and the derivative in the other coordinate times its fp32 error."""
    bi = B.bound_sum(r["gimg"], r["S_gimg"], "f32", r["L"][:, None] + 3)
    bf = B.gamma(8 * C + 2) * r["S_gflow"] + np.stack([r["dgx_dy"] * B.coord_delta(H), r["dgy_dx"] * B.coord_delta(W)], 1) \
        + B.ETA["f32"]
    return bi, bf


def replay_resample_bwd(dev, rec, g):
    a, img, flow = _resample_inputs(rec, g)
    N, C, H, W = img.shape
    gout = torch.randn(N, C, H, W, generator=g)
    r = F.resample2d_bwd(np64(img), np64(flow), np64(gout))
    bi, bf = resample_bwd_bounds(r, C, H, W)
    di, df, dg = img.to(dev), flow.to(dev), gout.to(dev)

    def launch():
        gimg, gflow = sentinel(img.shape, torch.float32, dev), sentinel(flow.shape, torch.float32, dev)
        call(rec["entry"], di, df, dg, gimg, gflow, N, C, H, W, a["kernel_size"])
        return gimg, gflow
    gimg, gflow = _twice("resample2d_bwd", launch, (None, "gflow"))      # (gimg: float atomics, any order)
    return {"gimg": assert_bound("gimg", *B.check_bound(np64(gimg), r["gimg"], bi), bi.shape),
            "gflow": assert_bound("gflow", *B.check_bound(np64(gflow), r["gflow"], bf), bf.shape)}


def channelnorm_bwd_inputs(rec, g):
    """x (pixel (0, 0, 0) all zero, times the record's ``scale``), out = the fp32-rounded fp64 norm, gout."""
    a = named_args(rec)
    N, C, H, W = a["N"], a["C"], a["H"], a["W"]
    x = torch.randn(N, C, H, W, generator=g) * rec.get("scale", 1.0)
    x[0, :, 0, 0] = 0
    out = torch.from_numpy(F.channelnorm(np64(x))).float()
    return a, x, out, torch.randn(N, 1, H, W, generator=g)


def replay_channelnorm_bwd(dev, rec, g):
    a, x, out, gout = channelnorm_bwd_inputs(rec, g)
    N, C, H, W = x.shape
    ref, _ = F.channelnorm_bwd(np64(x), np64(out), np64(gout))
    dx, do, dg = x.to(dev), out.to(dev), gout.to(dev)

    def launch():
        gin = sentinel(x.shape, torch.float32, dev)
        call(rec["entry"], dx, do, dg, gin, N, C, H, W, a["norm_deg"])
        return (gin,)
    gin, = _twice("channelnorm_bwd", launch, ("gin",))
    assert not bool(gin[0, :, 0, 0].ne(0).any()), "the gradient of an all-zero pixel is not zero"
    bnd = 3 * B.U32 * np.abs(ref) + B.ETA["f32"]        # one fp32 product, a double division, one cast
    return {"f32": assert_bound("channelnorm_bwd", *B.check_bound(np64(gin), ref, bnd), ref.shape)}


# ---------------------------------------------------------------------------------------------------------------------
# grouped losses
def _loss_tensors(rec, g, dtype, dev):
    """Per item: (a, b, mask) on the device and their fp64 copies.  Half operands are drawn exact in both formats."""
    items = []
    for it in rec["items"]:
        n = it["n"]
        if it["kind"] == 0:
            a, b, m = R.draw((n,), g), R.draw((n,), g), None
            items.append((a.to(dev, dtype), b.to(dev, dtype), None, np64(a), np64(b), None))
            continue
        a = R.draw((n,), g)
        b = R.draw((n,), g) if it["b"] else None
        m = (torch.rand(n // it["chw"] * it["hw"], generator=g) < 0.8).float() * \
            torch.rand(n // it["chw"] * it["hw"], generator=g).to(torch.bfloat16).float() if it["kind"] == 2 else None
        items.append((a.to(dev), None if b is None else b.to(dev), None if m is None else m.to(dev),
                      np64(a), None if b is None else np64(b), None if m is None else np64(m)))
    return items


def _loss_array(rec, ts, grads=None):
    from ir2rgb_amd import _lib
    arr = (_lib.LossItem * len(rec["items"]))()
    for i, (it, t) in enumerate(zip(rec["items"], ts)):
        e = arr[i]
        e.a, e.b, e.mask = t[0].data_ptr(), (t[1].data_ptr() if t[1] is not None else None), \
            (t[2].data_ptr() if t[2] is not None else None)
        e.ga = grads[i].data_ptr() if grads is not None and grads[i] is not None else None
        e.n, e.hw, e.chw, e.weight, e.target, e.kind, e.slot = (it["n"], it["hw"], it["chw"], it["weight"], it["target"],
                                                                 it["kind"], it["slot"])
    return arr


LOSS_BLOCKS = 512       # blocks of one loss launch (losses.hip), split over the items in proportion to n


def loss_chain(rec, i):
    """Longest fp32 chain of item i's slot: a lane's elements of its block slice (kind 0: 8 per uint4, four uint4 per
    trip), the wave / block tree (6 + 3), the finish pass (a thread's blocks, then 8 levels)."""
    ns = [it["n"] for it in rec["items"]]
    total = float(sum(ns))
    it = rec["items"][i]
    nb = min(int((LOSS_BLOCKS - len(ns)) * it["n"] / total) + 1, -(-it["n"] // 2048))
    if it["kind"] == 0:
        per = -(-(it["n"] // 8) // nb)
        lane = -(-per // 1024) * 4 * 8
    else:
        lane = -(-(-(-it["n"] // nb)) // 256)
    return lane + 9 + 2 + 8


def replay_loss_fwd(dev, rec, g):
    from ir2rgb_amd import _lib
    nslots = max(it["slot"] for it in rec["items"]) + 1
    out = {}
    for fmt, dtype, dt in DTYPES:
        if fmt != "bf16" and not any(it["kind"] == 0 for it in rec["items"]):
            continue        # the dtype only applies to the half operands of kind 0
        ts = _loss_tensors(rec, g, dtype, dev)
        ref = np.zeros(4)
        S = np.zeros(4)
        chain = 0
        for i, (it, t) in enumerate(zip(rec["items"], ts)):
            term, s = O.loss_term(it["kind"], t[3], t[4], t[5], it["target"], it["hw"], it["chw"])
            ref[it["slot"]] += it["weight"] / it["n"] * term.sum()
            S[it["slot"]] += abs(it["weight"]) / it["n"] * s.sum()
            chain = max(chain, loss_chain(rec, i))
        runs = []
        for _ in range(2):
            res = sentinel((4,), torch.float32, dev)
            part = torch.empty(_lib.lib().ir2rgb_loss_partial_elems(), dtype=torch.float32, device=dev)
            arr = _loss_array(rec, ts)
            rc = _lib.lib().ir2rgb_loss_multi_fwd(arr, len(rec["items"]), dt, part, res, _lib.current_stream(res))
            _lib.check(rc, "loss_multi_fwd")
            torch.cuda.synchronize()
            runs.append(res.cpu())
        assert torch.equal(bits(runs[0]), bits(runs[1])), f"{fmt}: loss slots differ between two runs"
        assert torch.isnan(runs[0][nslots:]).all(), f"{fmt}: a slot beyond the last named one was written"
        got = np64(runs[0][:nslots])
        out[fmt] = assert_bound(f"{fmt} slots", *B.check_bound(got, ref[:nslots], B.bound_rw(ref[:nslots], S[:nslots], "f32",
                                                                                          chain, 4)), (nslots,))
    return out


def replay_loss_bwd(dev, rec, g, mode=None):
    if mode is not None:
        return _ranged(dev, rec, mode)
    from ir2rgb_amd import _lib
    out = {}
    for fmt, dtype, dt in DTYPES:
        if fmt != "bf16" and not any(it["kind"] == 0 for it in rec["items"]):
            continue
        ts = _loss_tensors(rec, g, dtype, dev)
        gout = torch.randn(4, generator=g)
        grads = [(torch.full_like(t[0], float("nan")) if it["ga"] else None) for it, t in zip(rec["items"], ts)]
        arr = _loss_array(rec, ts, grads)
        rc = _lib.lib().ir2rgb_loss_multi_bwd(arr, len(rec["items"]), dt, gout.to(dev), _lib.current_stream(ts[0][0]))
        _lib.check(rc, "loss_multi_bwd")
        torch.cuda.synchronize()
        worst = 0.0
        for it, t, ga in zip(rec["items"], ts, grads):
            if ga is None:
                continue
            if it["kind"] == 0:     # sign(a - b) * half(gout * (weight / n)) exactly, the scale formed in fp32
                gs = np.float32(gout[it["slot"]].item()) * (np.float32(it["weight"]) / np.float32(it["n"]))
                want = torch.from_numpy(np.sign(t[3] - t[4])) * torch.tensor(float(gs)).to(dtype).double()
                exact(f"{fmt} L1 gradient", ga, want)
                continue
            gs = gout[it["slot"]].item() * it["weight"] / it["n"]
            ref = O.loss_grad(it["kind"], t[3], t[4], t[5], it["target"], it["hw"], it["chw"], gs)
            bnd = 4 * B.U32 * np.abs(ref) + B.ETA["f32"]
            worst = max(worst, assert_bound(f"{fmt} kind {it['kind']} gradient", *B.check_bound(np64(ga), ref, bnd), ref.shape))
        out[fmt] = worst
    return out


# ---------------------------------------------------------------------------------------------------------------------
# Adam: one table with one tensor per recorded (n, alignment) class; each array in a pool of its own, at a 16-byte
# offset (aligned) or a 4-byte one (not), with guard floats on both sides that must stay untouched
GUARD = 8


def _pool(n, aligned, fill, dev):
    off = GUARD if aligned else GUARD + 1
    pool = torch.full((n + 2 * GUARD + 4,), 777.0, dtype=torch.float32)
    pool[off:off + n] = fill
    pool = pool.to(dev)
    return pool, off


def replay_adam(dev, rec, g):
    from ir2rgb_amd import _lib
    E = _lib.lib().ir2rgb_adam_chunk_elems()
    lr, b1, b2, eps = rec["lr"], rec["beta1"], rec["beta2"], rec["eps"]
    b1f, b2f = float(np.float32(b1)), float(np.float32(b2))
    worst = 0.0
    for step in (1, 14):
        rows, blocks, pools, host = [], [], [], []
        for i, (n, aligned, _) in enumerate(rec["tensors"]):
            p = torch.randn(n, generator=g) * 0.05
            gr = torch.randn(n, generator=g) * 0.01
            m = torch.zeros(n) if step == 1 else torch.randn(n, generator=g) * 0.01
            v = torch.zeros(n) if step == 1 else torch.rand(n, generator=g) * 1e-4
            arrs = [_pool(n, aligned, t, dev) for t in (p, gr, m, v)]
            ptrs = [pl.data_ptr() + 4 * off for pl, off in arrs]
            assert all(q % 16 == 0 for q in ptrs) == bool(aligned)
            rows.append(ptrs + [n])
            blocks += [(i, c) for c in range(-(-n // E))]
            pools.append(arrs)
            host.append((p, gr, m, v))
        table = torch.tensor(rows, dtype=torch.int64, device=dev)
        blk = torch.tensor(blocks, dtype=torch.int32, device=dev)
        rc = _lib.lib().ir2rgb_adam_step(table, blk, len(blocks), lr, b1, b2, eps, step, _lib.current_stream(table))
        _lib.check(rc, "adam_step")
        torch.cuda.synchronize()
        for (n, aligned, _), arrs, (p, gr, m, v) in zip(rec["tensors"], pools, host):
            got = []
            for pl, off in arrs:
                h = pl.cpu()
                guard = torch.cat([h[:off], h[off + n:]])
                assert torch.all(guard == 777.0), f"n={n} aligned={aligned}: a pool guard was overwritten"
                got.append(h[off:off + n].double().numpy())
            p1, m1, v1, upd, Sm, ss, den = O.adam(*(t.double().numpy() for t in (p, gr, m, v)), lr, b1f, b2f, eps, step)
            bm = 4 * B.U32 * Sm + B.ETA["f32"]
            bv = 4 * B.U32 * v1 + B.ETA["f32"]
            bp = B.U32 * np.abs(p1) + 16 * B.U32 * upd + ss * bm / den + B.ETA["f32"]
            for name, gv, rv, bb in (("m", got[2], m1, bm), ("v", got[3], v1, bv), ("p", got[0], p1, bp)):
                worst = max(worst, assert_bound(f"step {step} n={n} aligned={aligned} {name}",
                                           *B.check_bound(gv, rv, bb), rv.shape))
            assert np.array_equal(got[1], gr.double().numpy()), "the gradient was written"
    return {"f32": worst}


REPLAY = {
    "ir2rgb_gather_f32": replay_gather,
    "ir2rgb_avgpool3s2": replay_avgpool,
    "ir2rgb_xexpand": replay_xexpand,
    "ir2rgb_xexpand_cx": replay_xexpand,
    "ir2rgb_xexpand_bwd": replay_xexpand_bwd,
    "ir2rgb_fold_reflect": replay_fold,
    "ir2rgb_thin_grad_expand": replay_thin_grad,
    "ir2rgb_flow_upsample_slice": replay_flow_up,
    "ir2rgb_nchw_f32_to_nhwc_half": replay_convert,
    "ir2rgb_nhwc_half_to_nchw_f32": replay_convert,
    "ir2rgb_nchw_f32_to_nhwc_half_slice": replay_convert,
    "ir2rgb_head_finish": replay_head_finish,
    "ir2rgb_head_finish_bwd": replay_head_finish_bwd,
    "ir2rgb_warp_blend_fwd": replay_warp_fwd,
    "ir2rgb_warp_blend_bwd": replay_warp_bwd,
    "ir2rgb_warp_diff_norm_fwd": replay_warp_diff_norm,
    "ir2rgb_channelnorm_fwd": replay_channelnorm,
    "ir2rgb_loss_multi_fwd": replay_loss_fwd,
    "ir2rgb_loss_multi_bwd": replay_loss_bwd,
    "ir2rgb_adam_step": replay_adam,
    "ir2rgb_correlation_fwd": replay_corr_fwd,
    "ir2rgb_correlation_bwd": replay_corr_bwd,
    "ir2rgb_correlation_nhwc_half": replay_corr_mfma,
    "ir2rgb_resample2d_fwd": replay_resample_fwd,
    "ir2rgb_resample2d_bwd": replay_resample_bwd,
    "ir2rgb_channelnorm_bwd": replay_channelnorm_bwd,
}
