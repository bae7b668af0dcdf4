"""fp64 replays of the convolution and BatchNorm launches (test-only), at records in the format of
tests/window_geometries.json: replay_forward and replay_wgrad for ``"kind": "conv"``, bn_case for ``"kind": "bn"``.

Each runs in bf16 and f16 from one fp64 reference (oracle/conv_ref.py, oracle/bn_ref.py): operands are drawn on values
exact in both formats.  Per-element bounds are oracle/bounds.py's and oracle/bn_ref.py's, fixed before anything runs.
Each returns {format: worst err/bound}.  tests/test_window_kernels_gpu.py runs them at the window's records,
tests/test_edge_bn_gpu.py runs bn_case and tests/test_edge_conv_gpu.py the two convolution replays at
oracle/edge_records.py's.
"""
import numpy as np
import torch

from oracle import bounds as B
from oracle import conv_ref as R
from oracle import window as WG
from oracle.replay import DTYPES, gen, hand


def _desc(d, dt):
    from ir2rgb_amd import conv as C
    from ir2rgb_amd._lib import ConvDesc
    return C.sealed(ConvDesc(*[d[f] if f != "dtype" else dt for f in WG.DESC_FIELDS]))


def _nhwc(t, dtype, dev):
    return t.to(dev, dtype).contiguous(memory_format=torch.channels_last)


def _rows_of(d, kernel, rows, P):
    """Pixel sets of the statistics rows: exact tiles for the single-class implicit GEMM (pixels in NHWC order, TP per
    tile, cut per sample when stats_per_sample); otherwise one set per sample group (per-sample rows) or one overall."""
    n, hw = d["N"], d["Hout"] * d["Wout"]
    sps = d["stats_per_sample"]
    if kernel == "conv_igemm_kernel" and not d["transposed"]:
        for tp in (64, 128, 256):
            per = -(-hw // tp)
            if (n * per if sps else -(-P // tp)) == rows:
                if sps:
                    return [np.arange(s * hw + t * tp, s * hw + min(hw, (t + 1) * tp)) for s in range(n)
                            for t in range(per)], "tile"
                return [np.arange(t * tp, min(P, (t + 1) * tp)) for t in range(rows)], "tile"
    if sps:
        return [np.arange(s * hw, (s + 1) * hw) for s in range(n)], "sample"
    return [np.arange(P)], "total"


def _group_rows(stats, d, mode, rows):
    """GPU statistics [rows, 2, C] summed (fp64) to the sets of _rows_of."""
    st = stats.double().cpu().numpy()
    if mode == "tile":
        return st
    if mode == "sample":
        return st.reshape(d["N"], rows // d["N"], 2, -1).sum(1)
    return st.sum(0, keepdims=True)


def _ranged(dev, rec, mode, build):
    """``mode`` of a replay: the inputs of oracle/range_cases.py (overflow / subnormal / nonfinite) under
    oracle.bounds.check_range, at an EDGE_RANGE record.  -> {format: worst err/bound, "counts": {format: the four counts}}."""
    from oracle import range_cases as RC
    return RC.run(dev, rec, mode, getattr(RC, build))


def replay_forward(dev, rec, mode=None):
    """A forward-type launch (conv2d_fwd with its split-K workspace, or conv2d_fwd_view on channel-slice buffers) with
    the recorded bias / statistics arguments.  -> worst err/bound per format, and per format of the statistics rows."""
    from ir2rgb_amd import conv as C
    if mode is not None:
        return _ranged(dev, rec, mode, "forward_case")
    d = rec["desc"]
    g = gen(rec)
    x = R.draw((d["N"], d["Cin"], d["Hin"], d["Win"]), g)
    w = R.draw(R.weight_shape(d), g, R.weight_scale(d))
    bias = R.draw((d["Cout"],), g) if rec["bias"] else None
    outs = {}
    for fmt, dtype, dt in DTYPES:
        desc = _desc(d, dt)
        # ("named": a hand-written record whose bias / statistics arguments send the launch past the kernel the query,
        # which sees the descriptor alone, names -- conv_dot_kernel and conv1x7_thin_kernel take neither)
        assert C.kernel_name(desc) == rec.get("named", rec["kernel"]), (fmt, C.kernel_name(desc), rec["kernel"])
        if d["pad_mode"] == C.PAD_REFLECT_ADJ:
            twin = _desc(dict(d, pad_mode=C.PAD_ZERO), dt)
            wp = C.pack_weight(twin, w.to(dev), adjoint=True)
        else:
            wp = C.pack_weight(desc, w.to(dev))
        b_dev = bias.to(dev) if bias is not None else None
        odt = torch.float32 if d["out_f32"] else dtype
        if rec["entry"] == "fwd":           # channel-slice launch of FlowNet2 (conv2d_fwd_view)
            ldx, ldy = d["ldx"] or d["Cin"], d["ldy"] or d["Cout"]
            xbuf = R.draw((d["N"], ldx, d["Hin"], d["Win"]), g)
            xbuf[:, d["ci_off"]:d["ci_off"] + d["Cin"]] = x
            xbuf = _nhwc(xbuf, dtype, dev)
            ybuf = _nhwc(R.draw((d["N"], ldy, d["Hout"], d["Wout"]), g), odt, dev)
            before = ybuf.clone()
            stats = torch.full((C.stats_rows(desc), 2, d["Cout"]), float("nan"), device=dev) if rec["stats"] else None
            C.conv2d_fwd_view(desc, xbuf, wp, b_dev, ybuf, stats)
            torch.cuda.synchronize()
            sl = slice(d["co_off"], d["co_off"] + d["Cout"])
            keep = torch.ones(ldy, dtype=torch.bool)
            keep[sl] = False
            assert torch.equal(ybuf[:, keep], before[:, keep]), "channel-slice launch wrote outside its channels"
            y = ybuf[:, sl]
        else:
            assert (C._lib.lib().ir2rgb_conv2d_fwd_workspace_bytes(desc) > 0) == rec["workspace"]
            y, stats = C.conv2d_fwd(desc, _nhwc(x, dtype, dev), wp, b_dev, want_stats=rec["stats"])
            torch.cuda.synchronize()
        outs[fmt] = (y.permute(0, 2, 3, 1).cpu(), stats)
    chain = B.chain_fwd(d)
    worst = {fmt: (0.0, None) for fmt, _, _ in DTYPES}
    P = d["N"] * d["Hout"] * d["Wout"]
    stat_acc = None
    if rec["stats"]:
        rows_of, mode = _rows_of(d, rec["kernel"], outs["bf16"][1].shape[0], P)
        row_id = np.empty(P, dtype=np.int64)
        for i, idx in enumerate(rows_of):
            row_id[idx] = i
        stat_acc = [np.zeros((len(rows_of), d["Cout"])) for _ in range(4)]
    hw = d["Hout"] * d["Wout"]
    for n, o0, o1, ref, S in R.forward_bands(d, x, w, bias):
        ref, S = ref.numpy(), S.numpy()
        for fmt, _, _ in DTYPES:
            ok, ratio, i, over = B.check(outs[fmt][0][n, o0:o1].double().numpy(), ref, S, "f32" if d["out_f32"] else fmt, chain)
            if ratio > worst[fmt][0]:
                worst[fmt] = (ratio, np.unravel_index(i, ref.shape))
            assert ok, (f"{fmt}: {over} elements over the bound (worst err/bound {ratio:.3g} at sample {n}, "
                        f"(y, x, c) = {np.unravel_index(i, ref.shape)} + ({o0}, 0, 0))")
        if stat_acc is not None:
            rid = row_id[n * hw + o0 * d["Wout"]:n * hw + o1 * d["Wout"]]
            terms = B.stats_terms(ref.reshape(-1, d["Cout"]), S.reshape(-1, d["Cout"]), chain)
            for acc, q in zip(stat_acc, terms):
                torch.from_numpy(acc).index_add_(0, torch.from_numpy(rid), torch.from_numpy(np.ascontiguousarray(q)))
    out = {fmt: worst[fmt][0] for fmt, _, _ in DTYPES}
    if stat_acc is not None:
        for fmt, _, _ in DTYPES:
            got = _group_rows(outs[fmt][1], d, mode, outs[fmt][1].shape[0])
            ok, ratio = B.check_stats(got, stat_acc)
            assert ok, f"{fmt}: statistics ({mode} rows) over the bound: worst err/bound {ratio:.3g}"
            out[f"stats[{mode}] {fmt}"] = ratio
    return out


def replay_wgrad(dev, rec, mode=None):
    """A weight gradient through conv2d_wgrad, plain and accumulating onto a seeded base."""
    from ir2rgb_amd import conv as C
    if mode is not None:
        return _ranged(dev, rec, mode, "wgrad_case")
    d = rec["desc"]
    g = gen(rec)
    x = hand("in", "x", R.draw((d["N"], d["Cin"], d["Hin"], d["Win"]), g))
    gy = hand("in", "gy", R.draw((d["N"], d["Cout"], d["Hout"], d["Wout"]), g))
    base = hand("in", "base", torch.randn(R.weight_shape(d), generator=g))
    ref, S = R.wgrad(d, x, gy)
    ref, S = ref.numpy(), S.numpy()
    chain = B.chain_wgrad(d)
    worst = {}
    for fmt, dtype, dt in DTYPES:
        desc = _desc(d, dt)
        xg, gg = _nhwc(x, dtype, dev), _nhwc(gy, dtype, dev)
        dw = C.conv2d_wgrad(desc, xg, gg)
        acc = base.to(dev).contiguous()
        C.conv2d_wgrad(desc, xg, gg, out=acc, accumulate=True)
        # (split slabs summed by the finish pass in a fixed order, no atomics: wgrad_mfma.hip) -- a repeat is bit-identical
        dw2 = C.conv2d_wgrad(desc, xg, gg)
        acc2 = base.to(dev).contiguous()
        C.conv2d_wgrad(desc, xg, gg, out=acc2, accumulate=True)
        torch.cuda.synchronize()
        assert torch.equal(dw, dw2) and torch.equal(acc, acc2), f"{fmt}: weight gradient not bit-reproducible"
        hand("out", f"{fmt} dw", dw)
        hand("out", f"{fmt} acc", acc)
        ok, ratio, i, over = B.check(dw.double().cpu().numpy(), ref, S, "f32", chain)
        assert ok, f"{fmt}: {over} weight-gradient elements over the bound (worst {ratio:.3g} at {np.unravel_index(i, ref.shape)})"
        bd = base.double().numpy()
        ok2, ratio2, i2, over2 = B.check(acc.double().cpu().numpy(), bd + ref, S + np.abs(bd), "f32", chain)
        assert ok2, f"{fmt}: accumulate=True: {over2} elements over the bound (worst {ratio2:.3g} at {np.unravel_index(i2, ref.shape)})"
        worst[fmt] = max(ratio, ratio2)
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# BatchNorm: every recorded launch of the window (finalize, fused finalize + apply, apply, backward) at its recorded
# rows / channels / pixel count / activation / residuals / accumulation, against oracle/bn_ref.py.
def _bn_data(P, C, g, shifted=False):
    """y [P, C] half-exact fp32 values with per-channel mean and spread (|mean| ~ 20 std when shifted)."""
    std = torch.rand(C, generator=g) * 1.5 + 0.5
    mu = 20 * std * torch.sign(torch.randn(C, generator=g)) if shifted else torch.randn(C, generator=g) * 0.5
    y = R.draw((P, C), g) * std + mu
    y = y.to(torch.bfloat16).float()
    y[y.abs() < 2.0 ** -14] = 0
    return y


def _vec(C, g, lo=None, hi=None):
    v = torch.rand(C, generator=g) * (hi - lo) + lo if lo is not None else torch.randn(C, generator=g) * 0.5
    return v.to(torch.bfloat16).float()


def _rows(y, R):
    """fp32 statistics rows of y over R contiguous pixel ranges (what the convolution hands BatchNorm)."""
    yd = y.double()
    parts = [torch.stack([c.sum(0), (c * c).sum(0)]) for c in torch.tensor_split(yd, R)]
    return torch.stack(parts).float()


def _pc(t, dtype, dev):
    """[P, C] -> the (1, C, 1, P) channels_last view the wrappers take (NHWC bytes = [P, C])."""
    P, C = t.shape
    return t.to(dev, dtype).contiguous().view(1, 1, P, C).permute(0, 3, 1, 2)


def bn_case(dev, rec, shifted=False, mode=None):
    """One BatchNorm record.  What a record can ask for beyond the window's launches (oracle/edge_records.py): the
    plain ir2rgb_bn_finalize entry; no conv_bias; evaluation mode (the frozen argument of ir2rgb_bn_finalize_ex, act | 16
    of ir2rgb_bn_bwd, also with act | 32); and, with the key "two_launch", the bit-identity of ir2rgb_bn_finalize_apply
    with ir2rgb_bn_finalize_ex + ir2rgb_bn_apply as a second assertion."""
    from ir2rgb_amd import _lib
    from oracle import bn_ref as BR
    if mode is not None:
        return _ranged(dev, rec, mode, "bn_case")
    a = rec["args"]
    g = gen(rec) if not shifted else torch.Generator().manual_seed(20)
    entry = rec["entry"]
    plain = entry == "ir2rgb_bn_finalize"
    if plain:           # the same arguments without conv_bias and frozen
        a = a[:6] + [False] + a[6:] + [0]
        entry = "ir2rgb_bn_finalize_ex"
    if entry == "ir2rgb_bn_bwd":
        P, C, act = a[10], a[11], a[12]
    elif entry == "ir2rgb_bn_apply":
        P, C, act = a[6], a[7], a[8]
    else:
        P, C = a[3], a[2]
        act = a[21] if entry == "ir2rgb_bn_finalize_apply" else 1
    y = hand("in", "y", _bn_data(P, C, g, shifted))
    yd = y.double().numpy()
    worst = {}
    for fmt, dtype, dt in DTYPES:
        def check(name, got, rb):
            ref, bnd = rb
            got = hand("out", f"{fmt} {name}", got).double().cpu().numpy().reshape(ref.shape)
            assert np.isfinite(got).all(), f"{fmt} {name}: non-finite"
            err = np.abs(got - ref)
            # (a sum whose every term is zero -- one pixel, a channel the activation switches off -- has the bound 0 and
            # must be exact: 0 / 0 is then a pass, anything else over a zero bound is not)
            r = np.divide(err, bnd, out=np.where(err > 0, np.inf, 0.0), where=bnd > 0).max()
            worst[fmt] = max(worst.get(fmt, 0.0), float(r))
            assert r <= 1.0, f"{fmt} {name}: worst err/bound {r:.3g}"
        f32 = dict(device=dev, dtype=torch.float32)
        stream = _lib.current_stream(torch.empty(1, device=dev))
        lib = _lib.lib()
        if entry in ("ir2rgb_bn_finalize_ex", "ir2rgb_bn_finalize_apply"):
            R_ = a[1]
            rows = _rows(y, R_)
            gamma, beta, cb = _vec(C, g, 0.5, 1.5), _vec(C, g), _vec(C, g) * 0.2
            rm, rv = _vec(C, g), _vec(C, g, 0.5, 2.0)
            mom, eps, upd = a[9], a[10], a[15]
            frozen = entry == "ir2rgb_bn_finalize_ex" and a[16]
            cb0 = cb.double().numpy() if a[6] else np.zeros(C)
            if frozen:
                ref = BR.finalize_frozen(gamma.double().numpy(), beta.double().numpy(), cb0, rm.double().numpy(),
                                         rv.double().numpy(), eps)
            else:
                ref = BR.finalize(rows.double().numpy(), float(P), gamma.double().numpy(), beta.double().numpy(),
                                  cb0, rm.double().numpy(), rv.double().numpy(), mom, eps, upd)
            dv = [hand("in", f"{fmt} statistics operand {i}", t).to(dev) for i, t in enumerate((rows, gamma, beta, cb, rm, rv))]
            if not a[6]:
                dv[3] = None
            outs = [torch.empty(C, **f32) for _ in range(4)]
            if plain:
                rc = lib.ir2rgb_bn_finalize(dv[0], R_, C, P, dv[1], dv[2], dv[4], dv[5], mom, eps, *outs, upd, stream)
                _lib.check(rc, "bn_finalize")
                z = None
            elif entry == "ir2rgb_bn_finalize_ex":
                rc = lib.ir2rgb_bn_finalize_ex(dv[0], R_, C, P, dv[1], dv[2], dv[3], dv[4], dv[5], mom, eps,
                                               *outs, upd, int(a[16]), stream)
                _lib.check(rc, "bn_finalize_ex")
                z = None
            else:
                res = [hand("in", f"{fmt} residual", R.draw((P, C), g)) if a[17 + i] else None for i in range(2)]
                x = y.to(dev, dtype)
                rdev = [r.to(dev, dtype) if r is not None else None for r in res]
                z = torch.empty_like(x)
                rc = lib.ir2rgb_bn_finalize_apply(dv[0], R_, C, P, dv[1], dv[2], dv[3], dv[4], dv[5], mom, eps,
                                                  *outs, upd, x, rdev[0], rdev[1], z, P, act, dt, stream)
                _lib.check(rc, "bn_finalize_apply")
            torch.cuda.synchronize()
            for name, t in zip(("scale", "shift", "mean", "invstd"), outs):
                check(name, t, ref[name] if name != "mean" else (ref["mean"][0], ref["mean"][1] + B.ETA["f32"]))
            if frozen:          # nothing is updated in evaluation mode
                assert torch.equal(dv[4].cpu(), rm) and torch.equal(dv[5].cpu(), rv), f"{fmt}: frozen finalize wrote the running statistics"
            else:
                check("running_mean", dv[4], ref["running_mean"])
                check("running_var", dv[5], ref["running_var"])
            if rec.get("two_launch"):       # the same through ir2rgb_bn_finalize_ex + ir2rgb_bn_apply, bit for bit
                dv2 = [t.to(dev) for t in (rows, gamma, beta, cb, rm, rv)]
                if not a[6]:
                    dv2[3] = None
                outs2 = [torch.empty(C, **f32) for _ in range(4)]
                z2 = torch.empty_like(z)
                _lib.check(lib.ir2rgb_bn_finalize_ex(dv2[0], R_, C, P, dv2[1], dv2[2], dv2[3], dv2[4], dv2[5], mom, eps,
                                                     *outs2, upd, 0, stream), "bn_finalize_ex")
                _lib.check(lib.ir2rgb_bn_apply(x, outs2[0], outs2[1], rdev[0], rdev[1], z2, P, C, act, dt, stream), "bn_apply")
                torch.cuda.synchronize()
                same = [torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(outs + dv[4:], outs2 + dv2[4:])]
                assert all(same) and torch.equal(z.view(torch.int16), z2.view(torch.int16)), \
                    f"{fmt}: fused finalize + apply differs from the two launches ({same})"
            if z is not None:
                rr = [r.double().numpy() if r is not None else None for r in res]
                check("z", z, BR.apply(yd, ref["scale"][0], ref["shift"][0], act, rr[0], rr[1], fmt,
                                        ref["scale"][1], ref["shift"][1]))
            if shifted:         # the window's next steps at this geometry: apply (ReLU) and backward
                z = torch.empty_like(y.to(dev, dtype))
                rc = lib.ir2rgb_bn_apply(y.to(dev, dtype), outs[0], outs[1], None, None, z, P, C, 1, dt, stream)
                _lib.check(rc, "bn_apply")
                torch.cuda.synchronize()
                sc, sh = outs[0].double().cpu().numpy(), outs[1].double().cpu().numpy()
                check("z", z, BR.apply(yd, sc, sh, 1, None, None, fmt))
                bn_bwd_check(dev, fmt, dtype, y, g, sc, sh, outs[2].double().cpu().numpy(),
                              outs[3].double().cpu().numpy(), 1, False, check)
        elif entry == "ir2rgb_bn_apply":
            scale, shift = hand("in", f"{fmt} scale", _vec(C, g, 0.5, 1.5)), hand("in", f"{fmt} shift", _vec(C, g))
            res = [hand("in", f"{fmt} residual", R.draw((P, C), g)) if a[3 + i] else None for i in range(2)]
            z = torch.empty(P, C, device=dev, dtype=dtype)
            rc = lib.ir2rgb_bn_apply(y.to(dev, dtype), scale.to(dev), shift.to(dev),
                                     *[r.to(dev, dtype) if r is not None else None for r in res], z, P, C, act, dt, stream)
            _lib.check(rc, "bn_apply")
            torch.cuda.synchronize()
            check("z", z, BR.apply(yd, scale.double().numpy(), shift.double().numpy(), act,
                                   *[r.double().numpy() if r is not None else None for r in res], fmt))
        else:
            has_scale = a[2]
            mean = y.double().mean(0)
            invstd = (1.0 / (y.double().var(0, unbiased=False) + 1e-5).sqrt()).float()
            mean = mean.float()
            gamma, beta = _vec(C, g, 0.5, 1.5), _vec(C, g)
            if act & 16:        # evaluation mode: the running statistics, not the batch's
                mean = (mean + _vec(C, g) * 0.25).to(torch.bfloat16).float()
                invstd = (1.0 / (_vec(C, g, 0.5, 2.0) + 1e-5).sqrt()).float()
            scale = (gamma * invstd) if has_scale else None
            shift = (beta - mean * scale) if has_scale else None
            bn_bwd_check(dev, fmt, dtype, y, g, None if scale is None else scale.double().numpy(),
                          None if shift is None else shift.double().numpy(), mean.double().numpy(),
                          invstd.double().numpy(), act & 15, bool(act & 32), check, frozen=bool(act & 16))
    return worst


def bn_bwd_check(dev, fmt, dtype, y, g, scale, shift, mean, invstd, act, acc, check, frozen=False):
    from ir2rgb_amd import autograd as AG
    from oracle import bn_ref as BR
    P, C = y.shape
    yd = y.double().numpy()
    gz = R.draw((P, C), g)
    gz[torch.from_numpy(~BR.sign_safe(yd, scale, shift))] = 0
    hand("in", f"{fmt} gz", gz)
    for name, v in (("scale", scale), ("shift", shift), ("mean", mean), ("invstd", invstd)):
        if v is not None:
            hand("in", f"{fmt} {name}", torch.from_numpy(np.asarray(v, dtype=np.float32)))
    base = (torch.randn(C, generator=g), torch.randn(C, generator=g)) if acc else None
    ref = BR.bwd(gz.double().numpy(), yd, scale, shift, mean, invstd, act, fmt,
                 None if base is None else (base[0].double().numpy(), base[1].double().numpy()), frozen=frozen)
    t = (lambda v: torch.from_numpy(np.asarray(v, dtype=np.float32)).to(dev) if v is not None else None)
    params = (base[0].to(dev), base[1].to(dev)) if acc else None
    norm = scale is not None
    gy, dgamma, dbeta = AG.bn_bwd(_pc(gz, dtype, dev), _pc(y, dtype, dev), t(scale), t(shift), t(mean) if norm else None,
                                  t(invstd) if norm else None, act | (16 if frozen else 0), params=params)
    torch.cuda.synchronize()
    check("gy", gy.permute(0, 2, 3, 1), ref["gy"])
    check("dbeta", dbeta, ref["dbeta"])
    if scale is not None:
        check("dgamma", dgamma, ref["dgamma"])
