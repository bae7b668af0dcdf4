"""fp64 references and per-element bounds of the BatchNorm kernels (test-only; see oracle/bounds.py for the form).

Arithmetic restated from include/ir2rgb_hip.h and read off the kernels:

* ``bn_finalize`` / ``bn_finalize_apply`` sum the fp32 statistics rows in double and derive mean, variance
  (E[y^2] - E[y]^2), invstd and the running statistics in double (pointwise.hip), then round to fp32 and take a few fp32
  products (scale = gamma * invstd, shift = beta - mean * scale).  Each fp32 result is therefore bounded by FIN = 8
  fp32 roundings of the magnitudes that enter it.
* ``bn_apply`` / the apply half: z = act(y * scale + shift) + res1 + res2 in fp32 from the kernel's own scale / shift,
  then rounded to the half format.
* ``bn_bwd``: g' = gz * act'(y * scale + shift); dbeta = sum g', dgamma = sum g' * yhat, summed per thread in fp32 over
  a pixel range and across ranges in double (backward.hip) -- bounded with the random-walk term of a chain of npix;
  gy = scale * (g' - dbeta / n - yhat * dgamma / n) in fp32 from the kernel's own sums, rounded to the half format
  (``gy_acc``: the error before that rounding, for oracle.bounds.check_range).

Elements whose pre-activation is so close to zero that fp32 and fp64 may disagree on its sign carry no gradient (the
caller zeroes gz there): the derivative of the activation is then not an arithmetic question.
"""
import numpy as np

from . import bounds as B

FIN = 8 * B.U32
ACT_NAMES = {0: "none", 1: "relu", 2: "leaky0.2"}


def act_np(a, act):
    return np.maximum(a, 0) if act == 1 else (np.where(a > 0, a, 0.2 * a) if act == 2 else a)


def dact_np(a, act):
    return (a > 0).astype(np.float64) if act == 1 else (np.where(a > 0, 1.0, 0.2) if act == 2 else np.ones_like(a))


def finalize(rows, count, gamma, beta, conv_bias, rm, rv, momentum, eps, updates):
    """rows [R, 2, C] fp32 (as float64), parameters [C] -> dict of fp64 references and bounds."""
    s1, s2 = rows[:, 0].sum(0), rows[:, 1].sum(0)
    mean = s1 / count
    ex2 = s2 / count
    var = np.maximum(ex2 - mean * mean, 0.0)
    # the double-precision sums: R additions of fp32 values, relative 2^-53 each -- far below FIN
    e_var = 4 * 2.0 ** -53 * rows.shape[0] * (np.abs(rows[:, 1]).sum(0) / count + mean * mean)
    invstd = 1.0 / np.sqrt(var + eps)
    e_inv = FIN * invstd + 0.5 * invstd * e_var / (var + eps)
    scale = gamma * invstd
    e_scale = FIN * np.abs(scale) + np.abs(gamma) * e_inv
    shift = beta - mean * scale
    e_shift = FIN * (np.abs(beta) + np.abs(mean * scale)) + np.abs(mean) * e_scale
    keep = (1.0 - momentum) ** updates
    # (count == 1: nn.BatchNorm2d refuses one value per channel; the kernels then keep the biased variance, 0)
    unbiased = var * count / (count - 1.0) if count > 1 else var
    rm_new = keep * rm + (1.0 - keep) * (mean + conv_bias)
    rv_new = keep * rv + (1.0 - keep) * unbiased
    return dict(mean=(mean, FIN * np.abs(mean)), invstd=(invstd, e_inv), scale=(scale, e_scale),
                shift=(shift, e_shift),
                running_mean=(rm_new, updates * FIN * (np.abs(rm) + np.abs(mean) + np.abs(conv_bias))),
                running_var=(rv_new, updates * FIN * (np.abs(rv) + unbiased) + e_var))


def finalize_frozen(gamma, beta, conv_bias, rm, rv, eps):
    """Evaluation mode (ir2rgb_bn_finalize_ex, frozen != 0): scale / shift / mean / invstd from the running statistics,
    formed in fp32 by the kernel (the sum, the root and the quotient of invstd, then products and differences: each result
    within FIN of the magnitudes that enter it, and the errors of its inputs carried through)."""
    invstd = 1.0 / np.sqrt(rv + eps)
    e_inv = FIN * invstd
    mu = rm - conv_bias
    e_mu = FIN * (np.abs(rm) + np.abs(conv_bias))
    scale = gamma * invstd
    e_scale = FIN * np.abs(scale) + np.abs(gamma) * e_inv
    shift = beta - mu * scale
    e_shift = FIN * (np.abs(beta) + np.abs(mu * scale)) + np.abs(mu) * e_scale + np.abs(scale) * e_mu
    return dict(mean=(mu, e_mu), invstd=(invstd, e_inv), scale=(scale, e_scale), shift=(shift, e_shift))


def apply_acc(y, scale, shift, act, res1, res2, e_scale=0.0, e_shift=0.0):
    """z = act(y * scale + shift) + res1 + res2: (ref, the error of the fp32 arithmetic before the result is rounded to
    the half format).  y / res [P, C] fp64 of half values; e_*: the error of the scale / shift the kernel used (0 when
    they are exact inputs)."""
    pre = y * scale + shift
    z = act_np(pre, act)
    mag = np.abs(y * scale) + np.abs(shift)
    e = np.abs(y) * e_scale + e_shift + 2 * B.U32 * mag
    for r in (res1, res2):
        if r is not None:
            z = z + r
            mag = mag + np.abs(r)
            e = e + B.U32 * mag
    return z, e


def apply(y, scale, shift, act, res1, res2, fmt, e_scale=0.0, e_shift=0.0):
    """(ref, bound) of apply_acc with the rounding to the half format and ETA."""
    z, e = apply_acc(y, scale, shift, act, res1, res2, e_scale, e_shift)
    u = B.U_OUT[fmt]
    return z, u * np.abs(z) + (1 + u) * e + B.ETA[fmt]


def sign_safe(y, scale, shift):
    """Mask of the elements whose pre-activation sign fp32 arithmetic cannot flip."""
    if scale is None:
        return y != 0
    pre = y * scale + shift
    return np.abs(pre) > 64 * B.U32 * (np.abs(y * scale) + np.abs(shift))


def bwd(gz, y, scale, shift, mean, invstd, act, fmt, base=None, frozen=False):
    """fp64 backward of act + BatchNorm (scale None: activation only).  gz / y [P, C] fp64 of half values, the vectors
    [C] fp64 of fp32 values.  base = (dgamma0, dbeta0) of the accumulating form.  frozen: evaluation-mode statistics
    (act | 16) -- mean / invstd are constants, gy = scale * g', the sums as in training.  -> dict name -> (ref, bound)."""
    n = gz.shape[0]
    chain = B.b_rw(n + 2)
    u = B.U_OUT[fmt]
    if scale is None:
        gp = gz * dact_np(y, act)
        db = gp.sum(0)
        # (the sum may be of the rounded half gy: + u_out per term)
        e_db = (chain + u) * np.abs(gp).sum(0)
        out = dict(gy=(gp, u * np.abs(gp) + 2 * B.U32 * np.abs(gp) + B.ETA[fmt]), dbeta=(db, e_db),
                   gy_acc=2 * B.U32 * np.abs(gp))
    else:
        gp = gz * dact_np(y * scale + shift, act)
        yhat = (y - mean) * invstd
        db, dg = gp.sum(0), (gp * yhat).sum(0)
        e_db = chain * np.abs(gp).sum(0) + FIN * np.abs(db)
        e_dg = chain * np.abs(gp * yhat).sum(0) + FIN * np.abs(dg)
        if frozen:
            gy = scale * gp
            e_gy = FIN * np.abs(gy)
        else:
            gy = scale * (gp - db / n - yhat * dg / n)
            mag = np.abs(scale) * (np.abs(gp) + np.abs(db) / n + np.abs(yhat * dg) / n)
            e_gy = np.abs(scale) * (e_db / n + np.abs(yhat) * e_dg / n) + FIN * mag
        out = dict(gy=(gy, u * np.abs(gy) + (1 + u) * e_gy + B.ETA[fmt]), dbeta=(db, e_db), dgamma=(dg, e_dg), gy_acc=e_gy)
    if base is not None:
        g0, b0 = base
        out["dbeta"] = (out["dbeta"][0] + b0, out["dbeta"][1] + B.U32 * (np.abs(b0) + np.abs(out["dbeta"][0])))
        if "dgamma" in out:
            out["dgamma"] = (out["dgamma"][0] + g0, out["dgamma"][1] + B.U32 * (np.abs(g0) + np.abs(out["dgamma"][0])))
    return out


def rejects(got, ref_bound):
    """True when some element of ``got`` is outside the bound (or not finite)."""
    ref, bnd = ref_bound
    got = np.asarray(got, dtype=np.float64)
    return bool((~np.isfinite(got)).any() or (np.abs(got - ref) > bnd).any())
