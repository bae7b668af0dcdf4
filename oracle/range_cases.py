"""The replays at f16's range edges and on planted inf / NaN (test-only): what ``mode=`` of replay_forward,
replay_wgrad and bn_case (oracle/replay_kernels.py) and of the layout-converter replay (oracle/replay_ops.py) runs.

A case is built on the CPU from a record of oracle/edge_records.py EDGE_RANGE, a mode and a number format:

    case(rec, mode, fmt) -> {"outs": [out, ...], "launch": fn(dev) -> {name: fp64 array}, ...}
    out = {"name", "ref", "acc", "fmt", "allow", "whole", "exact"}

``ref`` is the fp64 result of the operands *as stored* (after the cast to the format), evaluated under
np.errstate(all="ignore"); ``acc`` the accumulation part of the kernel's existing bound (oracle/bounds.py,
oracle/bn_ref.py) without the output rounding and without ETA -- both go to oracle.bounds.check_range.  Nothing in a
case needs a device before ``launch`` is called, so tests/test_range_cpu.py checks every case's liveness and runs the
emulated faulty stores against the same references the GPU test uses.

Modes (MODE_FMTS says which formats run):

* ``overflow`` (f16): today's draw times powers of two, split over the operands so that each stays finite in f16.  The
  exponent is the record's ``ek`` or, without one, the power of two that puts the 70 % quantile of |ref| at T = 65520:
  about 30 % of the outputs then must be inf and the rest finite.
* ``subnormal`` (f16): the gradient-like operand times 2^-SUB_K, cast to f16 (values of [2^-24, 2^-14), some rounded
  to 0), the reference from the cast values.  A fp32 bias of a forward record is scaled alike (it would otherwise lift
  every output out of the subnormal range); everything else as today.
* ``nonfinite`` (bf16, f16): one of +inf / -inf / NaN planted in one operand at the position the record's ``plant``
  names: (operand, position, value), positions FIRST (element 0), LAST (the last element: the ragged tail tile, the last
  pixel of a BatchNorm slab), BORDER (row 0, column 1: its receptive fields cross the reflected or padded border).

Liveness (``liveness``) is a condition on the references alone.
"""
import math

import numpy as np
import torch

from oracle import bn_ref as BR
from oracle import bounds as B
from oracle import conv_ref as R
from oracle.replay import differs, gen, rnd

MODES = ("overflow", "subnormal", "nonfinite")
MODE_FMTS = {"overflow": ("f16",), "subnormal": ("f16",), "nonfinite": ("bf16", "f16")}
TORCH = {"bf16": (torch.bfloat16, 1), "f16": (torch.float16, 2)}
VALUES = {"+inf": math.inf, "-inf": -math.inf, "nan": math.nan}
SUB_K = 18                      # N(0, 1) * 2^-18: all but the largest 2^-6 of the draw inside [2^-24, 2^-14)
QUANTILE = 0.7


def stored(t, fmt):
    """An fp32 tensor after the cast to the half format (what the kernel reads)."""
    return t.to(TORCH[fmt][0]).float()


def exponent(rec, ref, nonzero=False):
    """The power of two of the overflow mode: the record's, or the one that puts the QUANTILE of |ref| nearest T
    (nonzero: the 40 % quantile of the non-zero |ref|, for an output that is zero by construction at most elements)."""
    if "ek" in rec:
        return rec["ek"]
    a = np.abs(ref)
    q = float(np.quantile(a[a > 0], 0.4) if nonzero else np.quantile(a, QUANTILE))
    return int(round(math.log2(B.T_F16 / q)))


def searched_exponent(rec, ref_of):
    """For a result that is not homogeneous in the scaled operand (a shift or residuals stay as they are): the power of
    two k whose ref_of(k) has the share of |ref| > T nearest 1 - QUANTILE."""
    if "ek" in rec:
        return rec["ek"]
    share = {k: float((np.abs(ref_of(k)) > B.T_F16).mean()) for k in range(10, 24)}
    return min(share, key=lambda k: abs(share[k] - (1.0 - QUANTILE)))


def out(name, ref, acc, fmt, allow=None, whole=False, exact=False):
    return {"name": name, "ref": np.asarray(ref, dtype=np.float64), "acc": acc, "fmt": fmt, "allow": allow, "whole": whole,
            "exact": exact}


def plant(t, where, value):
    """Writes VALUES[value] into the fp32 tensor t at FIRST / LAST / BORDER ([.., row 0, column 1] of an NCHW tensor,
    channel C // 2) or at an explicit index tuple.  -> the index."""
    if where == "first":
        idx = (0,) * t.dim()
    elif where == "last":
        idx = tuple(s - 1 for s in t.shape)
    elif where == "border":
        idx = (0, t.shape[1] // 2, 0, min(1, t.shape[3] - 1))
    else:
        idx = tuple(where)
    t[idx] = VALUES[value]
    return idx


# ---------------------------------------------------------------------------------------------------------------------
# liveness and the check of a launched case
def counts_of(o):
    """check_range's four counts of an output, from the reference alone."""
    with np.errstate(all="ignore"):
        return B.check_range(rnd(o["ref"], o["fmt"]), o["ref"], o["acc"], o["fmt"])[3]


def liveness(case, mode):
    """(ok, text): the mode's condition on the case's references."""
    outs = case["outs"]
    if mode == "overflow":
        half = [counts_of(o) for o in outs if o["fmt"] == "f16"]
        n = sum(o["ref"].size for o in outs if o["fmt"] == "f16")
        if not n:
            return False, "no f16 output"
        mi, mf, un = (sum(c[k] for c in half) / n for k in ("must_inf", "must_finite", "undecided"))
        return mi >= 0.10 and mf >= 0.10 and un <= 0.02, f"must-inf {mi:.3f} must-finite {mf:.3f} undecided {un:.4f}"
    if mode == "subnormal":
        refs = [np.abs(o["ref"]).ravel() for o in outs if o["fmt"] == "f16"]
        if not refs:            # only fp32 consumers of the subnormal gradient: the operand itself carries the condition
            frac = case["subnormal_operand"]
            return frac >= 0.25, f"subnormal operand fraction {frac:.3f}"
        a = np.concatenate(refs)
        frac = float(((a >= 2.0 ** -23) & (a < 2.0 ** -15)).mean())
        return frac >= 0.25, f"subnormal fraction {frac:.3f}"
    total = 0
    for o in outs:
        nf = int((~np.isfinite(o["ref"])).sum())
        total += nf
        if nf == o["ref"].size and not o["whole"]:
            return False, f"{o['name']}: the whole output is non-finite"
        if o["whole"] and nf != o["ref"].size:
            return False, f"{o['name']}: said to be non-finite as a whole, {nf} of {o['ref'].size} are"
    return total > 0, f"{total} non-finite reference elements"


def check_out(o, got):
    """-> (ok, ratio, index, counts) of one output: check_range, or bit-equality with the rounded reference."""
    if o["exact"]:          # replay.exact's comparison: the bits of the fp64 value rounded to nearest even
        dt = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[o["fmt"]]
        t = (lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dt))
        same = ~differs(t(got), t(o["ref"])).numpy()
        cnt = counts_of(o)
        return bool(same.all()), 0.0 if same.all() else math.inf, int(np.argmin(same.ravel())), cnt
    with np.errstate(all="ignore"):
        return B.check_range(got, o["ref"], o["acc"], o["fmt"], o["allow"])


def run(dev, rec, mode, build):
    """Launches build(rec, mode, fmt) for the mode's formats and holds every output to check_range.
    -> {format: worst err/bound} and, under "counts", the four counts summed over the outputs per format."""
    worst, counts = {}, {}
    for fmt in MODE_FMTS[mode]:
        c = build(rec, mode, fmt)
        ok, text = liveness(c, mode)
        assert ok, f"{fmt} {mode}: the reference is not live: {text}"
        got = c["launch"](dev)
        tot = dict.fromkeys(("must_inf", "must_finite", "undecided", "ref_nonfinite"), 0)
        w = 0.0
        for o in c["outs"]:
            g = np.asarray(got[o["name"]], dtype=np.float64).reshape(o["ref"].shape)
            ok, ratio, i, cnt = check_out(o, g)
            at = np.unravel_index(i, o["ref"].shape)
            print(f"{fmt} {mode} {o['name']}: worst err/bound {ratio:.4g} {cnt}")
            assert ok, (f"{fmt} {mode} {o['name']}: first failing element {tuple(int(v) for v in at)}: got {g[at]!r}, "
                        f"reference {o['ref'][at]!r}; {cnt}")
            w = max(w, ratio)
            for k in tot:
                tot[k] += cnt[k]
        if "after" in c:
            c["after"](got, fmt)
        worst[fmt] = w
        counts[fmt] = tot
    worst["counts"] = counts
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# forward-type convolution launches (also every data gradient: a forward launch with adjoint weights)
def forward_case(rec, mode, fmt):
    from oracle import replay_kernels as RK
    d = rec["desc"]
    assert rec["entry"] == "fwd_ws"
    g = gen(rec)
    x = R.draw((d["N"], d["Cin"], d["Hin"], d["Win"]), g)
    w = R.draw(R.weight_shape(d), g, R.weight_scale(d))
    bias = R.draw((d["Cout"],), g) if rec["bias"] else None
    ofmt = "f32" if d["out_f32"] else fmt
    note = {}
    with np.errstate(all="ignore"):
        if mode == "overflow":
            ref0, _ = R.forward(d, x, w, bias)
            k = exponent(rec, ref0.numpy())
            kx = k // 2
            x, w = x * 2.0 ** kx, w * 2.0 ** (k - kx)
            bias = bias * 2.0 ** k if bias is not None else None
            assert torch.isfinite(stored(x, fmt)).all() and torch.isfinite(stored(w, fmt)).all()
            note["ek"] = k
        elif mode == "subnormal":
            x = stored(x * 2.0 ** -SUB_K, fmt)
            bias = bias * 2.0 ** -SUB_K if bias is not None else None
        else:
            operand, where, value = rec["plant"]
            note["at"] = plant({"x": x, "w": w, "bias": bias}[operand], where, value)
        ref, S = R.forward(d, x, w, bias)
    ref, S = ref.numpy(), S.numpy()
    chain = B.chain_fwd(d)
    ax = np.abs(x.numpy())
    sub = float(((ax >= 2.0 ** -24) & (ax < 2.0 ** -14)).mean())

    def launch(dev):
        from ir2rgb_amd import conv as C
        dtype, dt = TORCH[fmt]
        desc = RK._desc(d, dt)
        assert C.kernel_name(desc) == rec.get("named", rec["kernel"]), (fmt, C.kernel_name(desc), rec["kernel"])
        if d["pad_mode"] == C.PAD_REFLECT_ADJ:
            wp = C.pack_weight(RK._desc(dict(d, pad_mode=C.PAD_ZERO), dt), w.to(dev), adjoint=True)
        else:
            wp = C.pack_weight(desc, w.to(dev))
        y, stats = C.conv2d_fwd(desc, RK._nhwc(x, dtype, dev), wp, bias.to(dev) if bias is not None else None,
                                want_stats=rec["stats"])
        torch.cuda.synchronize()
        return {"y": y.permute(0, 2, 3, 1).double().cpu().numpy(), "stats": stats}

    def after(got, fmt_):
        """The fp32 statistics rows, taken before the half store, under today's check_stats (overflow and subnormal)."""
        if not rec["stats"] or mode == "nonfinite":
            return
        P = d["N"] * d["Hout"] * d["Wout"]
        rows_of, how = RK._rows_of(d, rec["kernel"], got["stats"].shape[0], P)
        terms = B.stats_terms(ref.reshape(-1, d["Cout"]), S.reshape(-1, d["Cout"]), chain)
        acc = [np.stack([q[idx].sum(0) for idx in rows_of]) for q in terms]
        ok, ratio = B.check_stats(RK._group_rows(got["stats"], d, how, got["stats"].shape[0]), acc)
        print(f"{fmt_} {mode} statistics ({how} rows): worst err/bound {ratio:.4g}")
        assert ok, f"{fmt_} {mode}: statistics ({how} rows) over the bound: worst err/bound {ratio:.3g}"

    with np.errstate(all="ignore"):
        acc = B.b_rw(chain) * S
    return {"outs": [out("y", ref, acc, ofmt)], "launch": launch, "after": after, "note": note, "subnormal_operand": sub}


# ---------------------------------------------------------------------------------------------------------------------
# weight gradients: fp32 consumers of half gradients (plain, and accumulating onto a seeded base)
def wgrad_case(rec, mode, fmt):
    from oracle import replay_kernels as RK
    assert mode != "overflow"
    d = rec["desc"]
    g = gen(rec)
    x = R.draw((d["N"], d["Cin"], d["Hin"], d["Win"]), g)
    gy = R.draw((d["N"], d["Cout"], d["Hout"], d["Wout"]), g)
    base = torch.randn(R.weight_shape(d), generator=g)
    note = {}
    if mode == "subnormal":
        gy = stored(gy * 2.0 ** -SUB_K, fmt)
    else:
        operand, where, value = rec["plant"]
        note["at"] = plant({"x": x, "gy": gy}[operand], where, value)
    with np.errstate(all="ignore"):
        ref, S = R.wgrad(d, x, gy)
        ref, S = ref.numpy(), S.numpy()
        bd = base.double().numpy()
        b = B.b_rw(B.chain_wgrad(d))
        outs = [out("dw", ref, b * S, "f32"), out("acc", bd + ref, b * (S + np.abs(bd)), "f32")]
    ag = np.abs(gy.numpy())

    def launch(dev):
        from ir2rgb_amd import conv as C
        dtype, dt = TORCH[fmt]
        desc = RK._desc(d, dt)
        xg, gg = RK._nhwc(x, dtype, dev), RK._nhwc(gy, dtype, dev)
        dw = C.conv2d_wgrad(desc, xg, gg)
        acc = base.to(dev).contiguous()
        C.conv2d_wgrad(desc, xg, gg, out=acc, accumulate=True)
        torch.cuda.synchronize()
        return {"dw": dw.double().cpu().numpy(), "acc": acc.double().cpu().numpy()}

    return {"outs": outs, "launch": launch, "note": note,
            "subnormal_operand": float(((ag >= 2.0 ** -24) & (ag < 2.0 ** -14)).mean())}


# ---------------------------------------------------------------------------------------------------------------------
# BatchNorm: apply, fused finalize + apply, backward
def _bn_shape(rec):
    a = rec["args"]
    e = rec["entry"]
    if e == "ir2rgb_bn_bwd":
        return a[10], a[11], a[12]
    if e == "ir2rgb_bn_apply":
        return a[6], a[7], a[8]
    return a[3], a[2], a[21] if e == "ir2rgb_bn_finalize_apply" else 0


def bn_case(rec, mode, fmt):
    return {"ir2rgb_bn_apply": _apply_case, "ir2rgb_bn_finalize_apply": _fused_case,
            "ir2rgb_bn_finalize_ex": _fused_case, "ir2rgb_bn_bwd": _bwd_case}[rec["entry"]](
        rec, mode, fmt)


def _apply_case(rec, mode, fmt):
    from oracle import replay_kernels as RK
    assert mode != "subnormal"
    a = rec["args"]
    P, C, act = _bn_shape(rec)
    g = gen(rec)
    y = RK._bn_data(P, C, g)
    scale, shift = RK._vec(C, g, 0.5, 1.5), RK._vec(C, g)
    res = [R.draw((P, C), g) if a[3 + i] else None for i in range(2)]
    rr = [r.double().numpy() if r is not None else None for r in res]
    note = {}
    with np.errstate(all="ignore"):
        if mode == "overflow":          # through a large scale
            k = searched_exponent(rec, lambda k: BR.apply_acc(y.double().numpy(), scale.double().numpy() * 2.0 ** k,
                                                              shift.double().numpy(), act, *rr)[0])
            scale = scale * 2.0 ** k
            note["ek"] = k
        else:
            _, where, value = rec["plant"]
            note["at"] = plant(y, where, value)
        z, e = BR.apply_acc(y.double().numpy(), scale.double().numpy(), shift.double().numpy(), act, *rr)

    def launch(dev):
        from ir2rgb_amd import _lib
        dtype, dt = TORCH[fmt]
        zt = torch.empty(P, C, device=dev, dtype=dtype)
        rc = _lib.lib().ir2rgb_bn_apply(y.to(dev, dtype), scale.to(dev), shift.to(dev),
                                        *[r.to(dev, dtype) if r is not None else None for r in res], zt, P, C, act, dt,
                                        _lib.current_stream(zt))
        _lib.check(rc, "bn_apply")
        torch.cuda.synchronize()
        return {"z": zt.double().cpu().numpy()}

    return {"outs": [out("z", z, e, fmt)], "launch": launch, "note": note}


def _fused_case(rec, mode, fmt):
    """ir2rgb_bn_finalize_apply, and ir2rgb_bn_finalize_ex (no x, no z: the statistics-row plant only).  overflow: gamma
    times 2^ek.  nonfinite: the plant in x (one element; the statistics rows
    are those of the clean data) or in a statistics row ("rows": the sum of channel C // 2 in the last row is NaN), which
    under torch's semantics makes the channel's mean, variance, scale and shift -- and with them every pixel of the
    channel and its running statistics -- NaN."""
    from oracle import replay_kernels as RK
    assert mode != "subnormal"
    a = rec["args"]
    fused = rec["entry"] == "ir2rgb_bn_finalize_apply"
    assert fused or (mode == "nonfinite" and rec["plant"][0] == "rows" and not a[16])
    P, C, act = _bn_shape(rec)
    R_, mom, eps, upd = a[1], a[9], a[10], a[15]
    g = gen(rec)
    y = RK._bn_data(P, C, g)
    rows = RK._rows(y, R_)
    gamma, beta, cb = RK._vec(C, g, 0.5, 1.5), RK._vec(C, g), RK._vec(C, g) * 0.2
    rm, rv = RK._vec(C, g), RK._vec(C, g, 0.5, 2.0)
    res = [R.draw((P, C), g) if fused and a[17 + i] else None for i in range(2)]
    rr = [r.double().numpy() if r is not None else None for r in res]
    x = y.clone()
    note = {}
    cb0 = cb.double().numpy() if a[6] else np.zeros(C)

    def fin(gm):
        return BR.finalize(rows.double().numpy(), float(P), gm.double().numpy(), beta.double().numpy(), cb0,
                           rm.double().numpy(), rv.double().numpy(), mom, eps, upd)
    with np.errstate(all="ignore"):
        if mode == "overflow":
            def z_of(k):
                f0 = fin(gamma * 2.0 ** k)
                return BR.apply_acc(x.double().numpy(), f0["scale"][0], f0["shift"][0], act, *rr)[0]
            k = searched_exponent(rec, z_of)
            gamma = gamma * 2.0 ** k
            note["ek"] = k
        else:
            operand, where, value = rec["plant"]
            if operand == "rows":
                rows[R_ - 1, 0, C // 2] = VALUES[value]
                note["at"] = (R_ - 1, 0, C // 2)
            else:
                note["at"] = plant(x, where, value)
        f = fin(gamma)
        z, e = BR.apply_acc(x.double().numpy(), f["scale"][0], f["shift"][0], act, *rr, f["scale"][1], f["shift"][1])
        e = np.where(np.isfinite(z), e, 0.0)
    names = ("scale", "shift", "mean", "invstd", "running_mean", "running_var")
    outs = [out("z", z, e, fmt)] if fused else []
    for n in names:
        r_, b_ = f[n]
        with np.errstate(all="ignore"):
            outs.append(out(n, r_, np.where(np.isfinite(r_), b_, 0.0), "f32"))

    def launch(dev):
        from ir2rgb_amd import _lib
        dtype, dt = TORCH[fmt]
        dv = [t.to(dev) for t in (rows, gamma, beta, cb, rm, rv)]
        if not a[6]:
            dv[3] = None
        o4 = [torch.empty(C, device=dev, dtype=torch.float32) for _ in range(4)]
        if not fused:
            rc = _lib.lib().ir2rgb_bn_finalize_ex(dv[0], R_, C, P, dv[1], dv[2], dv[3], dv[4], dv[5], mom, eps, *o4, upd, 0,
                                                  _lib.current_stream(o4[0]))
            _lib.check(rc, "bn_finalize_ex")
            torch.cuda.synchronize()
            return {n: t.double().cpu().numpy() for n, t in zip(names, o4 + dv[4:])}
        xd = x.to(dev, dtype)
        zt = torch.empty_like(xd)
        rdev = [r.to(dev, dtype) if r is not None else None for r in res]
        rc = _lib.lib().ir2rgb_bn_finalize_apply(dv[0], R_, C, P, dv[1], dv[2], dv[3], dv[4], dv[5], mom, eps, *o4, upd, xd,
                                                 rdev[0], rdev[1], zt, P, act, dt, _lib.current_stream(zt))
        _lib.check(rc, "bn_finalize_apply")
        torch.cuda.synchronize()
        got = {"z": zt.double().cpu().numpy()}
        for n, t in zip(names, o4 + dv[4:]):
            got[n] = t.double().cpu().numpy()
        return got

    return {"outs": outs, "launch": launch, "note": note}


def _bwd_case(rec, mode, fmt):
    """ir2rgb_bn_bwd.  overflow: gz, scale and shift times 2^(ek / 2) each (the activation's mask is unchanged; the
    bias-only form has no operand to split over and is not run).  subnormal: gz.  nonfinite: the plant in gz at the first /
    last element whose pre-activation is positive (torch's ReLU gradient is a select, so a masked plant does not exist
    for it), or in y (activations without a zero branch only: act 0 and LeakyReLU)."""
    from oracle import replay_kernels as RK
    a = rec["args"]
    P, C, act = _bn_shape(rec)
    frozen, accum, act = bool(act & 16), bool(act & 32), act & 15
    assert not accum
    has_scale = a[2]
    g = gen(rec)
    y = RK._bn_data(P, C, g)
    mean = y.double().mean(0)
    invstd = (1.0 / (y.double().var(0, unbiased=False) + 1e-5).sqrt()).float()
    mean = mean.float()
    gamma, beta = RK._vec(C, g, 0.5, 1.5), RK._vec(C, g)
    if frozen:
        mean = (mean + RK._vec(C, g) * 0.25).to(torch.bfloat16).float()
        invstd = (1.0 / (RK._vec(C, g, 0.5, 2.0) + 1e-5).sqrt()).float()
    scale = (gamma * invstd) if has_scale else None
    shift = (beta - mean * scale) if has_scale else None
    gz = R.draw((P, C), g)
    yd = y.double().numpy()
    sd = (lambda v: None if v is None else v.double().numpy())
    safe = BR.sign_safe(yd, sd(scale), sd(shift))
    gz[torch.from_numpy(~safe)] = 0
    note = {}

    def ref_of():
        return BR.bwd(gz.double().numpy(), y.double().numpy(), sd(scale), sd(shift), sd(mean), sd(invstd), act, fmt,
                      frozen=frozen)
    with np.errstate(all="ignore"):
        if mode == "overflow":
            assert has_scale
            r0 = ref_of()
            k = exponent(rec, r0["gy"][0])
            kz = k // 2
            gz = gz * 2.0 ** kz
            scale, shift = scale * 2.0 ** (k - kz), shift * 2.0 ** (k - kz)
            assert torch.isfinite(stored(gz, fmt)).all()
            note["ek"] = k
        elif mode == "subnormal":
            gz = stored(gz * 2.0 ** -SUB_K, fmt)
        else:
            operand, where, value = rec["plant"]
            pre = yd * sd(scale) + sd(shift) if has_scale else yd
            if operand == "gz":
                c = 0 if where == "first" else C - 1
                live = np.nonzero((pre[:, c] > 0) & safe[:, c])[0]
                at = (int(live[0] if where == "first" else live[-1]), c)
                gz[at] = VALUES[value]
            else:
                assert act != 1
                at = plant(y, where, value)
            note["at"] = at
        r = ref_of()
    outs = []
    for name in ("gy", "dbeta", "dgamma"):
        if name not in r:
            continue
        ref = r[name][0]
        with np.errstate(all="ignore"):
            acc = r["gy_acc"] if name == "gy" else r[name][1]
            acc = np.where(np.isfinite(ref) & np.isfinite(acc), acc, 0.0)
        allow = None
        if name == "gy" and frozen and mode == "nonfinite":
            # Listed exception.  Evaluation mode drops the batch terms of gy by passing 1 / n = 0 to the kernels that
            # form  scale * (g' - dbeta / n - yhat * dgamma / n)  (ir2rgb_bn_bwd, backward.hip): the terms are
            # multiplied by zero, not skipped, so a non-finite dbeta / dgamma makes the whole channel of the plant NaN
            # where torch's gy = scale * g' is non-finite at the planted pixel only.  More propagating than torch.
            allow = np.zeros(ref.shape, dtype=bool)
            allow[:, note["at"][1]] = True
        outs.append(out(name, ref, acc, fmt if name == "gy" else "f32", allow=allow))

    def launch(dev):
        from ir2rgb_amd import autograd as AG
        dtype, _ = TORCH[fmt]
        t = (lambda v: v.float().to(dev) if v is not None else None)
        gy, dgamma, dbeta = AG.bn_bwd(RK._pc(gz, dtype, dev), RK._pc(y, dtype, dev), t(scale), t(shift),
                                      t(mean) if has_scale else None, t(invstd) if has_scale else None,
                                      act | (16 if frozen else 0))
        torch.cuda.synchronize()
        got = {"gy": gy.permute(0, 2, 3, 1).double().cpu().numpy().reshape(P, C), "dbeta": dbeta.double().cpu().numpy()}
        if has_scale:
            got["dgamma"] = dgamma.double().cpu().numpy()
        return got

    ag = np.abs(gz.numpy())
    return {"outs": outs, "launch": launch, "note": note,
            "subnormal_operand": float(((ag >= 2.0 ** -24) & (ag < 2.0 ** -14)).mean())}


# ---------------------------------------------------------------------------------------------------------------------
# the three layout converters: bit-equality with the rounded reference in every mode
def convert_case(rec, mode, fmt):
    from oracle import replay_ops as RO
    from oracle import window_ops_ref as O
    a = RO.named_args(rec)
    N, C, H, W = a["N"], a["C"], a["H"], a["W"]
    g = gen(rec)
    x = torch.randn(N, C, H, W, generator=g)
    note = {}
    if mode == "overflow":              # N(0, 1) * 2^16: a third beyond 65520, and values of the undecided band
        x = x * 2.0 ** 16
        n = min(4, x.numel())
        x.view(-1)[:n] = torch.tensor([65519.0, 65520.0, -65520.0, 65521.0])[:n]
    elif mode == "subnormal":
        x = x * 2.0 ** -SUB_K
    else:
        note["at"] = [plant(x, wh, v) for wh, v in (("first", "nan"), ("last", "+inf"))]
        if x.numel() > 2:
            x.view(-1)[x.numel() // 2] = -math.inf
    entry = rec["entry"]
    if entry == "ir2rgb_nhwc_half_to_nchw_f32":
        x = stored(x, fmt)              # its input is the half tensor: every stored value must come back exactly
        ref = x.double().numpy()
        ofmt = "f32"
    else:
        with np.errstate(all="ignore"):
            ref = O.nchw_to_nhwc(x.double().numpy(), a.get("act", 0))
        ofmt = fmt

    def launch(dev):
        return {"out": RO.launch_convert(dev, rec, x, fmt)}

    ax = np.abs(x.numpy())
    return {"outs": [out("out", ref, 0.0, ofmt, exact=True)], "launch": launch, "note": note,
            "subnormal_operand": float(((ax >= 2.0 ** -24) & (ax < 2.0 ** -14)).mean())}


# ---------------------------------------------------------------------------------------------------------------------
# the other gradient-path and half-store entry points (oracle/replay_ops.py)
def _sub_frac(t):
    a = np.abs(np.asarray(t, dtype=np.float64))
    return float(((a >= 2.0 ** -24) & (a < 2.0 ** -14)).mean())


def _mode_input(x, mode, fmt, rec, note, k_over=16, half_in=False):
    """The one varied operand of an op case: times 2^k_over, times 2^-SUB_K, or with the record's plant."""
    if mode == "overflow":
        x = x * 2.0 ** rec.get("ek", k_over)
    elif mode == "subnormal":
        x = x * 2.0 ** -SUB_K
    else:
        _, where, value = rec["plant"]
        note["at"] = plant(x, where, value)
    return stored(x, fmt) if half_in else x


def xexpand_case(rec, mode, fmt):
    """ir2rgb_xexpand: fp32 planes -> half rows, a copy: bit-equality in every mode."""
    from oracle import replay_ops as RO
    from oracle import window_ops_ref as O
    a = RO.named_args(rec)
    N, Cin, H, W, Wout, KW, s_, p_, pm = (a[k] for k in "N Cin H W Wout KW stride_w pad_w pad_mode".split())
    note = {}
    x = _mode_input(torch.randn(N, Cin, H, W, generator=gen(rec)), mode, fmt, rec, note)
    with np.errstate(all="ignore"):
        ref = O.xexpand(x.double().numpy(), Wout, KW, s_, p_, pm, 64)

    def launch(dev):
        dtype, dt = TORCH[fmt]
        y = RO.sentinel((N, H, Wout, 64), dtype, dev)
        RO.call(rec["entry"], x.to(dev), y, N, Cin, H, W, Wout, KW, s_, p_, pm, dt)
        torch.cuda.synchronize()
        return {"out": RO.np64(y)}
    return {"outs": [out("out", ref, 0.0, fmt, exact=True)], "launch": launch, "note": note, "subnormal_operand": _sub_frac(x)}


def xexpand_bwd_case(rec, mode, fmt):
    """ir2rgb_xexpand_bwd: the half gradient dxe summed into fp32 planes."""
    from oracle import replay_ops as RO
    from oracle import window_ops_ref as O
    a = RO.named_args(rec)
    N, Cin, H, W, Wout, KW, s_, p_, pm = (a[k] for k in "N Cin H W Wout KW stride_w pad_w pad_mode".split())
    note = {}
    dxe = _mode_input(R.draw((N, H, Wout, 64), gen(rec)), mode, fmt, rec, note, half_in=True)
    with np.errstate(all="ignore"):
        ref, cnt = O.xexpand_bwd(dxe.double().numpy(), Cin, W, KW, s_, p_, pm)
        S, _ = O.xexpand_bwd(np.abs(dxe.double().numpy()), Cin, W, KW, s_, p_, pm)
        acc = np.where(np.isfinite(S), B.gamma(int(cnt.max())) * S, 0.0)

    def launch(dev):
        dtype, dt = TORCH[fmt]
        din = RO.sentinel((N, Cin, H, W), torch.float32, dev)
        RO.call(rec["entry"], dxe.to(dev, dtype), din, N, Cin, H, W, Wout, KW, s_, p_, pm, dt)
        torch.cuda.synchronize()
        return {"din": RO.np64(din)}
    return {"outs": [out("din", ref, acc, "f32")], "launch": launch, "note": note, "subnormal_operand": _sub_frac(dxe)}


def fold_case(rec, mode, fmt):
    """ir2rgb_fold_reflect: half in, half out, sums of at most four terms (no overflow mode: an output beyond 65520
    would need inputs beyond it)."""
    from oracle import replay_ops as RO
    from oracle import window_ops_ref as O
    a = RO.named_args(rec)
    N, H, W, C, ph, pw = (a[k] for k in "N H W C pad_h pad_w".split())
    note = {}
    dxpad = R.draw((N, H + 2 * ph, W + 2 * pw, C), gen(rec))
    if mode == "nonfinite":
        _, where, value = rec["plant"]
        note["at"] = plant(dxpad, where, value)
    else:
        dxpad = stored(dxpad * 2.0 ** -SUB_K, fmt)
    with np.errstate(all="ignore"):
        ref, cnt = O.fold_reflect(dxpad.double().numpy(), ph, pw)
        S, _ = O.fold_reflect(np.abs(dxpad.double().numpy()), ph, pw)
        acc = np.where(np.isfinite(S), B.gamma(int(cnt.max())) * S, 0.0)

    def launch(dev):
        dtype, dt = TORCH[fmt]
        dx = RO.sentinel((N, H, W, C), dtype, dev)
        RO.call(rec["entry"], dxpad.to(dev, dtype), dx, N, H, W, C, ph, pw, dt)
        torch.cuda.synchronize()
        return {"dx": RO.np64(dx)}
    return {"outs": [out("dx", ref, acc, fmt)], "launch": launch, "note": note}


def thin_grad_case(rec, mode, fmt):
    """ir2rgb_thin_grad_expand: the fp32 logit gradient copied into two zero-padded half tensors (bit-equality) and
    summed per channel (dbias, fp32)."""
    from oracle import replay_ops as RO
    a = RO.named_args(rec)
    N, Cout, H, W = a["N"], a["Cout"], a["H"], a["W"]
    note = {}
    gz = _mode_input(torch.randn(N, Cout, H, W, generator=gen(rec)), mode, fmt, rec, note)
    want = np.zeros((N, H, W, 8))
    with np.errstate(all="ignore"):
        want[..., :Cout] = gz.double().permute(0, 2, 3, 1).numpy()
        ref = gz.double().sum((0, 2, 3)).numpy()
        S = gz.double().abs().sum((0, 2, 3)).numpy()
        acc = np.where(np.isfinite(S), B.b_rw(-(-N * H * W // 256) + 8) * S, 0.0)

    def launch(dev):
        dtype, dt = TORCH[fmt]
        g64, g8 = RO.sentinel((N, H, W, 64), dtype, dev), RO.sentinel((N, H, W, 8), dtype, dev)
        db = RO.sentinel((Cout,), torch.float32, dev)
        RO.call(rec["entry"], gz.to(dev), g64, g8, db, N, Cout, H, W, dt)
        torch.cuda.synchronize()
        assert not bool(g64[..., 8:].ne(0).any()), f"{fmt}: g64 channels >= 8 are not zero"
        return {"g8": RO.np64(g8), "g64": RO.np64(g64[..., :8]), "dbias": RO.np64(db)}
    return {"outs": [out("g8", want, 0.0, fmt, exact=True), out("g64", want, 0.0, fmt, exact=True),
                     out("dbias", ref, acc, "f32")], "launch": launch, "note": note, "subnormal_operand": _sub_frac(gz)}


def flow_up_case(rec, mode, fmt):
    """ir2rgb_flow_upsample_slice: 8 fp32 MACs and a bias per output, stored as half (heads.hip, its own _Float16 cast)."""
    from oracle import replay_ops as RO
    from oracle import window_ops_ref as O
    a = RO.named_args(rec)
    N, h, w, ld, off = a["N"], a["h"], a["w"], a["ld"], a["c_off"]
    g = gen(rec)
    note = {}
    x = R.draw((N, 2, h, w), g, 4.0)
    wt = R.draw((2, 2, 4, 4), g, 0.5)
    bias = R.draw((2,), g) if a["bias"] else None
    with np.errstate(all="ignore"):
        if mode == "overflow":
            r0, _ = O.flow_upsample(x.double().numpy(), wt.double().numpy(), None)
            k = exponent(rec, r0)
            x = x * 2.0 ** k
            note["ek"] = k
        elif mode == "subnormal":
            x = x * 2.0 ** -SUB_K
            bias = bias * 2.0 ** -SUB_K if bias is not None else None
        else:
            _, where, value = rec["plant"]
            note["at"] = plant(x, where, value)
        ref, S = O.flow_upsample(x.double().numpy(), wt.double().numpy(), None if bias is None else bias.double().numpy())
        ref, S = ref.transpose(0, 2, 3, 1), S.transpose(0, 2, 3, 1)
        acc = np.where(np.isfinite(S), B.gamma(9) * S, 0.0)

    def launch(dev):
        dtype, dt = TORCH[fmt]
        buf = torch.zeros(N, 2 * h, 2 * w, ld, dtype=dtype, device=dev)
        RO.call(rec["entry"], x.to(dev), wt.to(dev), None if bias is None else bias.to(dev), buf, N, h, w, ld, off, dt)
        torch.cuda.synchronize()
        keep = torch.ones(ld, dtype=torch.bool)
        keep[off:off + 2] = False
        assert not bool(buf[..., keep].ne(0).any()), f"{fmt}: flow up-sampler wrote outside its channels"
        return {"out": RO.np64(buf[..., off:off + 2])}
    return {"outs": [out("out", ref, acc, fmt)], "launch": launch, "note": note}


def head_bwd_case(rec, mode, fmt):
    """ir2rgb_head_finish_bwd: dT (half, heads.hip's own _Float16 cast) and dbias (fp32) from the fp32 gradient gout."""
    from oracle import replay_ops as RO
    from oracle import window_ops_ref as O
    a = RO.named_args(rec)
    N, H, W, Cout, KH, CT, pad, acts, mul = (a[k] for k in "N H W Cout KH CT pad_h acts mul".split())
    g = gen(rec)
    note = {}
    pre = torch.randn(N, Cout, H, W, generator=g, dtype=torch.float64) * 2
    o64 = np.empty(pre.shape)
    for co in range(Cout):
        nb = O.nibble(acts, co)
        p = pre[:, co].numpy()
        o64[:, co] = np.tanh(p) if nb == 1 else (1 / (1 + np.exp(-p)) if nb == 2 else p * mul)
    outv = torch.from_numpy(o64).float()
    gout = torch.randn(N, Cout, H, W, generator=g)
    with np.errstate(all="ignore"):
        if mode == "overflow":
            r0 = O.head_finish_bwd(gout.double().numpy(), outv.double().numpy(), Cout, KH, CT, pad, acts, mul)[0]
            k = exponent(rec, r0[..., :Cout * KH])
            gout = gout * 2.0 ** k
            note["ek"] = k
        else:
            gout = _mode_input(gout, mode, fmt, rec, note)
        ref, dbias, S, Sb = O.head_finish_bwd(gout.double().numpy(), outv.double().numpy(), Cout, KH, CT, pad, acts, mul)

    def launch(dev):
        from ir2rgb_amd import _lib
        dtype, dt = TORCH[fmt]
        rows = _lib.lib().ir2rgb_head_finish_bwd_rows(N, H, W)
        dT = RO.sentinel((N, H, W, CT), dtype, dev)
        db = RO.sentinel((Cout,), torch.float32, dev)
        part = torch.empty(rows * 8, dtype=torch.float32, device=dev)
        RO.call(rec["entry"], gout.to(dev), outv.to(dev), dT, db, part, N, H, W, Cout, KH, CT, pad, acts, mul, dt)
        torch.cuda.synchronize()
        assert not bool(dT[..., Cout * KH:].ne(0).any()), f"{fmt}: dT channels >= Cout*KH are not zero"
        return {"dT": RO.np64(dT[..., :Cout * KH]), "dbias": RO.np64(db)}
    with np.errstate(all="ignore"):
        acc_t = np.where(np.isfinite(S), (6 * B.U32 + B.b_rw(3)) * S, 0.0)[..., :Cout * KH]
        from ir2rgb_amd import _lib
        rows = _lib.lib().ir2rgb_head_finish_bwd_rows(N, H, W)         # (a host query: no device)
        chain = -(-N * H * W // (rows * 256)) + 256 + -(-rows // 32) + 32      # as replay_head_finish_bwd
        acc_b = np.where(np.isfinite(Sb), (6 * B.U32 + B.b_rw(chain)) * Sb, 0.0)
    return {"outs": [out("dT", ref[..., :Cout * KH], acc_t, fmt), out("dbias", dbias, acc_b, "f32")], "launch": launch,
            "note": note, "subnormal_operand": _sub_frac(gout)}


def corr_case(rec, mode, fmt):
    """ir2rgb_correlation_nhwc_half, out mode 1 (the half cost volume with its LeakyReLU).  overflow: both feature maps
    times 2^(ek / 2); nonfinite: the plant in the first map."""
    from oracle import flow_ops_ref as F
    from oracle import replay_ops as RO
    assert mode != "subnormal"
    a = RO.named_args(rec)
    N, C, H, W = a["N"], a["C"], a["H"], a["W"]
    lda, offa, ldb, offb, ldo, offo, slope = (a[k] for k in "lda offa ldb offb ldo offo slope".split())
    g = gen(rec)
    note = {}
    f1, f2 = R.draw((N, C, H, W), g), R.draw((N, C, H, W), g)
    with np.errstate(all="ignore"):
        if mode == "overflow":
            r0, _ = F.correlation(f1.double().numpy(), f2.double().numpy(), 20, 1, 20, 1, 2)
            k = exponent(rec, RO.leaky(r0, slope), nonzero=True)     # (displacements beyond the image are exact zeros)
            f1, f2 = f1 * 2.0 ** (k // 2), f2 * 2.0 ** (k - k // 2)
            assert torch.isfinite(stored(f1, fmt)).all() and torch.isfinite(stored(f2, fmt)).all()
            note["ek"] = k
        else:
            _, where, value = rec["plant"]
            note["at"] = plant(f1, where, value)
        ref, S = F.correlation(f1.double().numpy(), f2.double().numpy(), 20, 1, 20, 1, 2)
        ref = RO.leaky(ref, slope)
        acc = np.where(np.isfinite(S), B.b_rw(C + 2) * S, 0.0)
    allow = None
    if mode == "nonfinite":
        # Listed exception.  A displacement that leaves the image is an exact zero in the fp64 reference, which skips it;
        # the kernel multiplies the planted pixel with the zero-filled border of the other map (correlation_mfma.hip), as
        # the zero-padded product of the reference operator does, and 0 * inf is NaN: all 441 displacements of the
        # planted pixel may be non-finite.
        n_, _, y_, x_ = note["at"]
        allow = np.zeros(ref.shape, dtype=bool)
        allow[n_, :, y_, x_] = True

    def launch(dev):
        dtype, dt = TORCH[fmt]
        bufs = []
        for f, ld, off in ((f1, lda, offa), (f2, ldb, offb)):
            t = torch.zeros((N, H, W, ld), dtype=dtype)
            t[..., off:off + C] = f.permute(0, 2, 3, 1).to(dtype)
            bufs.append(t.to(dev))
        o = RO.sentinel((N, H, W, ldo), dtype, dev)
        RO.call(rec["entry"], bufs[0], lda, offa, bufs[1], ldb, offb, o, 1, ldo, offo, slope, N, C, H, W, dt)
        torch.cuda.synchronize()
        return {"out": RO.np64(o[..., offo:offo + 441].permute(0, 3, 1, 2))}
    return {"outs": [out("out", ref, acc, fmt, allow=allow)], "launch": launch, "note": note}


def loss_bwd_case(rec, mode, fmt):
    """ir2rgb_loss_multi_bwd, the root of the scaled backward pass: kind 0 stores sign(a - b) * f2h(gout * weight / n),
    the fp32 kinds their gradient in fp32.  overflow: gout = 2^ek * (1, 2, .5, 4) per slot, so that weight / n decides
    per item which side of 65520 it lands on; subnormal: gout = 2^-ek * the same (a scale of 2^16 over n ~ 2^24, restated
    with the record's n);
    nonfinite: the record's value in gout[plant slot].  torch's gradient is the product sign(a - b) * g, NaN where
    a = b under a non-finite g."""
    from oracle import replay_ops as RO
    from oracle import window_ops_ref as O
    g = gen(rec)
    dtype, dt = TORCH[fmt]
    note = {}
    ts = RO._loss_tensors(rec, g, dtype, torch.device("cpu"))
    base = torch.tensor([1.0, 2.0, 0.5, 4.0])
    if mode == "overflow":
        gout = base * 2.0 ** rec["ek"][0]
    elif mode == "subnormal":
        gout = base * 2.0 ** -rec["ek"][1]
    else:
        gout = torch.randn(4, generator=g)
        _, slot, value = rec["plant"]
        gout[slot] = VALUES[value]
        note["at"] = slot
    outs = []

    def whole(it):          # every element of an item's gradient carries its slot's gout: the record's plant says which
        return mode == "nonfinite" and it["slot"] == rec["plant"][1]
    with np.errstate(all="ignore"):
        for i, (it, t) in enumerate(zip(rec["items"], ts)):
            if not it["ga"]:
                continue
            if it["kind"] == 0:     # the scale formed in fp32 and rounded to the half format once, then signed
                gs = np.float32(gout[it["slot"]].item()) * (np.float32(it["weight"]) / np.float32(it["n"]))
                outs.append(out(f"ga{i}", np.sign(t[3] - t[4]) * float(gs), 0.0, fmt, exact=True, whole=whole(it)))
            else:
                gs = gout[it["slot"]].item() * it["weight"] / it["n"]
                ref = O.loss_grad(it["kind"], t[3], t[4], t[5], it["target"], it["hw"], it["chw"], gs)
                outs.append(out(f"ga{i}", ref, np.where(np.isfinite(ref), 4 * B.U32 * np.abs(ref), 0.0), "f32", whole=whole(it)))

    def launch(dev):
        from ir2rgb_amd import _lib
        dts = [tuple(None if v is None else v.to(dev) for v in t[:3]) + t[3:] for t in ts]
        grads = [(torch.full_like(t[0], float("nan")) if it["ga"] else None) for it, t in zip(rec["items"], dts)]
        arr = RO._loss_array(rec, dts, grads)
        rc = _lib.lib().ir2rgb_loss_multi_bwd(arr, len(rec["items"]), dt, gout.to(dev), _lib.current_stream(dts[0][0]))
        _lib.check(rc, "loss_multi_bwd")
        torch.cuda.synchronize()
        return {f"ga{i}": RO.np64(ga) for i, ga in enumerate(grads) if ga is not None}
    # kind 0 is the half store: the liveness of the overflow and subnormal modes is over its outputs
    return {"outs": outs, "launch": launch, "note": note}


OP_CASES = {"ir2rgb_xexpand": xexpand_case, "ir2rgb_xexpand_bwd": xexpand_bwd_case, "ir2rgb_fold_reflect": fold_case,
            "ir2rgb_thin_grad_expand": thin_grad_case, "ir2rgb_flow_upsample_slice": flow_up_case,
            "ir2rgb_head_finish_bwd": head_bwd_case, "ir2rgb_correlation_nhwc_half": corr_case,
            "ir2rgb_loss_multi_bwd": loss_bwd_case}


def build_for(rec):
    if rec["entry"] in OP_CASES:
        return OP_CASES[rec["entry"]]

    if rec["kind"] == "conv":
        return wgrad_case if rec["entry"] == "wgrad" else forward_case
    if rec["kind"] == "bn":
        return bn_case
    return convert_case
