"""Per-element error bounds of the half-precision MFMA kernels against an fp64 reference (test-only).

A kernel result ``got`` of an exact value ``ref`` is accepted when, element by element,

    |got - ref| <= u_out * |ref| + (1 + u_out) * b * S + eta

* ``u_out``: unit roundoff of the stored output (2^-8 bf16, 2^-11 f16, 0 when the kernel writes fp32);
* ``S``: the same linear operation on absolute values (sum of |a*b| over the element's products, + |bias|);
* ``b``: the fp32 accumulation term of the element's summation chain (below);
* ``eta``: the smallest normal number of the output format -- covers rounding (or flushing) at the underflow edge.

Operands are bf16 values inside f16's normal range, so every product of two of them is exact in fp32 (8 + 8 or 11 + 11
significand bits <= 24) and only the additions round.

The accumulation term ``b``
---------------------------
The worst-case form gamma_L = L * 2^-24 is rigorous for any summation order but grows with the chain length L: for the
weight gradients at 512 x 1024 (L = 524288 pixels) it is 0.031 * S, about 14 times a typical |ref| of random operands
(|ref| ~ sqrt(L) * rms(ab), S = L * E|ab|), which no fault could exceed.  Even the random-walk bound below is ~16 % of a
typical |ref| there: at that size it catches gross faults only; the fault tests (test_kernel_bounds_cpu.py) show what
it rejects at a 99k-pixel weight gradient.  The bf16 / f16 MFMA's
own accumulation has not been measured here (the f32-input MFMA is a round-to-nearest fma chain with error
~3.5e-7 * S at K = 4096, i.e. 0.09 * sqrt(K) * 2^-24 * S).  We therefore use the random-walk form

    b = C_RW * sqrt(L) * 2^-24,   C_RW = 8,

with L the longest chain the kernel's tiling gives (``chain_*`` below).  C_RW is fixed before any comparison: a
round-to-nearest chain over random operands stays near 0.1 * sqrt(L) * 2^-24 * S (the f32 MFMA figure), and even a
chain that truncated at every addition (errors of one sign, 2^-23 each, on partial sums that grow like sqrt(k))
accumulates ~2 * sqrt(L) * 2^-24 * S, four times inside the bound.  The form is for random operands (what these tests
draw); it is not a worst case over adversarial data.
"""
import math

import numpy as np

U32 = 2.0 ** -24
C_RW = 8.0
U_OUT = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11, "f32": 0.0}
ETA = {"bf16": 2.0 ** -126, "f16": 2.0 ** -14, "f32": 2.0 ** -126}
MAX_SPLIT = 256                # weight gradients: at most 256 pixel splits added in the finish pass (wgrad_mfma.hip)
MAX_TILE_PIXELS = 256          # statistics rows: one per pixel tile of at most 256 pixels (conv_mfma.hip tile_pixels)


def b_rw(chain):
    return C_RW * math.sqrt(chain) * U32


def chain_fwd(desc):
    """Forward-type launches: K = Cin * taps products (the split-K form adds its two partials: + 1), + bias (+ 1)."""
    taps = desc["kh"] * desc["kw"]
    return desc["Cin"] * taps + 2


def chain_wgrad(desc):
    """Weight gradients: one product per output pixel of the batch, split over at most MAX_SPLIT segments whose fp32
    partial sums the finish pass adds (+ the base of the accumulating form)."""
    return desc["N"] * desc["Hout"] * desc["Wout"] + MAX_SPLIT + 1


def bound(ref, S, fmt, chain):
    u = U_OUT[fmt]
    return u * np.abs(ref) + (1.0 + u) * b_rw(chain) * S + ETA[fmt]


def check(got, ref, S, fmt, chain):
    """(ok, worst err/bound ratio, index of the worst element, count over the bound).  Non-finite values fail."""
    got = np.asarray(got, dtype=np.float64)
    bnd = bound(ref, S, fmt, chain)
    if not np.isfinite(got).all():
        return False, math.inf, int(np.argmin(np.isfinite(got).ravel())), int((~np.isfinite(got)).sum())
    r = np.abs(got - ref) / bnd
    i = int(np.argmax(r))
    over = int((r > 1.0).sum())
    return over == 0, float(r.ravel()[i]), i, over


def stats_terms(ref, S, chain):
    """Per-pixel terms of the statistics-row check.  ``ref``/``S`` [P, C] fp64.  The kernel sums fp32 outputs v
    (|v - ref| <= e = b * S) over the at most MAX_TILE_PIXELS pixels of a row, and squares them for the second half:
      |sum v   - sum ref  | <= sum e + b_t * sum (|ref| + e)
      |sum v^2 - sum ref^2| <= sum e (2 |ref| + e) + b_t * sum (|ref| + e)^2,   b_t = b_rw(MAX_TILE_PIXELS + 3)
    (+3: the square's rounding and the four per-wave partials).  Returns (ref, ref^2, bound_sum, bound_sq) [P, C],
    to be summed over each row's pixels."""
    e = b_rw(chain) * S
    bt = b_rw(MAX_TILE_PIXELS + 3)
    a = np.abs(ref) + e
    return ref, ref * ref, e + bt * a, e * (2 * np.abs(ref) + e) + bt * a * a


def check_stats(got, acc):
    """got [R, 2, C] statistics rows (fp64), acc = the four stats_terms summed per row.  -> (ok, worst ratio)."""
    rs, rq, bs, bq = acc
    if not np.isfinite(got).all():
        return False, math.inf
    ratio = max((np.abs(got[:, 0] - rs) / bs).max(), (np.abs(got[:, 1] - rq) / bq).max())
    return bool(ratio <= 1.0), float(ratio)


# ---------------------------------------------------------------------------------------------------------------------
# Non-convolution entry points of the window (oracle/replay_ops.py, oracle/window_ops_ref.py).  Constants fixed
# before any comparison:
#
# * short fp32 sums of L terms (reflect folds, the xexpand adjoint, 3x3 pooling, the 8-MAC flow up-sampler, the KH + 1
#   terms of head_finish): the worst case gamma_L = L * 2^-24 (rigorous for any order), then the output rounding:
#       |got - ref| <= u_out |ref| + (1 + u_out) gamma_L S + eta                                   (bound_sum)
# * activations (head_finish): the pre-activation error propagates through |f'(pre)|, and the device tanhf / expf add
#   their own error.  That ulp error was NOT measured on gfx950; C_ACT = 4 ulps of fp32 (2^-23 each) is a margin over
#   the few ulps such implementations promise; the sigmoid's 1/(1 + e) adds two roundings, counted in C_ACT too.
#       |got - ref| <= |f'(pre)| gamma_{KH+1} S_pre + (C_ACT * 2^-23 + 2^-24) |ref| + eta_f32          (bound_act)
# * long deterministic reductions (head_finish_bwd / thin_grad_expand bias gradients, loss slots): the random-walk term
#   above with the kernel's chain, plus c_term roundings (2^-24 each) in forming each summand:
#       |got - ref| <= u_out |ref| + (1 + u_out) (c_term 2^-24 + b_rw(chain)) S + eta             (bound_rw)
# * bilinear sampling (warp_blend): the sampling coordinate ix = ((gx + 1) W - 1) / 2 is formed in fp32 from
#   gx = linspace(-1, 1, W)[x] + flow / ((W - 1) / 2), |gx| <= ~2: about ten roundings of magnitude <= 2 in gx
#   (the linspace step and product, the division, the sum), scaled by W / 2, and three more of magnitude <= 3 W / 2
#   in the unnormalisation.  DELTA_COORD = 16 rounds that to  delta = 16 * 2^-24 * (W + 1)  (1.0e-3 at W = 1024).
#   The value error is |d out / d ix| delta_x + |d out / d iy| delta_y on top of C_AR = 8 roundings of the arithmetic
#   (products of the four weights, the blend) over S.
C_ACT = 4.0
C_AR = 8.0
DELTA_COORD = 16.0


def gamma(L):
    return L * U32


def coord_delta(n):
    return DELTA_COORD * U32 * (n + 1)


def bound_sum(ref, S, fmt, terms):
    u = U_OUT[fmt]
    return u * np.abs(ref) + (1.0 + u) * gamma(terms) * S + ETA[fmt]


def bound_act(ref, slope, S_pre, terms):
    return slope * gamma(terms) * S_pre + (C_ACT * 2 * U32 + U32) * np.abs(ref) + ETA["f32"]


def bound_rw(ref, S, fmt, chain, c_term):
    u = U_OUT[fmt]
    return u * np.abs(ref) + (1.0 + u) * (c_term * U32 + b_rw(chain)) * S + ETA[fmt]


def check_bound(got, ref, bnd):
    """check() against a precomputed per-element bound: (ok, worst ratio, index of the worst, count over)."""
    got = np.asarray(got, dtype=np.float64)
    if not np.isfinite(got).all():
        return False, math.inf, int(np.argmin(np.isfinite(got).ravel())), int((~np.isfinite(got)).sum())
    r = np.abs(got - ref) / bnd
    i = int(np.argmax(r))
    over = int((r > 1.0).sum())
    return over == 0, float(r.ravel()[i]), i, over


# ---------------------------------------------------------------------------------------------------------------------
# The range-aware check (tests/test_range_cpu.py, tests/test_range_gpu.py): f16's overflow and underflow edges and
# planted inf / NaN, which check() and check_bound() refuse outright or cover with ETA.
#
# * rounding: max(u_out |ref|, H) with H half the subnormal spacing of the output format -- f16: 2^-25, and no ETA, so
#   a store that flushes a subnormal |ref| > H + the accumulation term fails.  bf16 and f32 keep u_out |ref| + ETA
#   (their subnormals are fp32's).
# * overflow (f16 outputs): T_F16 = 65520 is the round-to-nearest-even midpoint between 65504 and 2^16.  The fp32 value
#   v the kernel rounds is within the accumulation term e of ref, and the rounding of v is not in doubt: an element whose
#   |ref| - e > T must be inf of ref's sign, one whose |ref| + e < T must be finite and inside the bound, and in between
#   either is accepted.  (The rounding term is deliberately not part of that band: with it the band would reach 2^16 and
#   a store that rounded toward zero at the top -- 65521 -> 65504 -- could not be told from a correct one.)
# * a non-finite reference element (fp64 evaluation of planted operands under torch's semantics) wants a non-finite
#   result: for +-inf that inf or NaN, for NaN anything non-finite.  ``allow`` marks the finite-reference elements where
#   the record lists by rule that the kernel may be non-finite as well.
T_F16 = 65520.0
H_SUB = {"f16": 2.0 ** -25}


def range_masks(ref, bnd_acc, fmt):
    """What check_range pins, from the reference alone: (ref finite, the bound of a finite result, must be inf, must be
    finite); the finite elements in neither mask are undecided."""
    ref = np.asarray(ref, dtype=np.float64)
    u = U_OUT[fmt]
    fin = np.isfinite(ref)
    with np.errstate(all="ignore"):
        aref = np.where(fin, np.abs(ref), 0.0)
        acc = np.where(fin, np.broadcast_to(np.asarray(bnd_acc, dtype=np.float64), ref.shape), 0.0)
        assert np.isfinite(acc).all(), "the accumulation bound of a finite reference element is not finite"
        rnd = np.maximum(u * aref, H_SUB[fmt]) if fmt in H_SUB else u * aref + ETA[fmt]
        bnd = rnd + (1.0 + u) * acc
        if fmt == "f16":
            return fin, bnd, fin & (aref - acc > T_F16), fin & (aref + acc < T_F16)
        return fin, bnd, np.zeros(ref.shape, dtype=bool), fin


def check_range(got, ref, bnd_acc, fmt, allow=None):
    """got against the fp64 ``ref`` of the operands as stored.  ``bnd_acc``: the accumulation part of the kernel's bound
    (b_rw / gamma terms times S) without u_out |ref| and without ETA.  -> (ok, worst err/bound over the elements that
    must be finite -- inf when any element fails --, index of the worst or first failing element, counts of
    {must_inf, must_finite, undecided, ref_nonfinite})."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    with np.errstate(all="ignore"):
        fin, bnd, must_inf, must_fin = range_masks(ref, bnd_acc, fmt)
        und = fin & ~must_inf & ~must_fin
        gfin = np.isfinite(got)
        inside = gfin & (np.abs(got - np.where(fin, ref, 0.0)) <= bnd)
        right_inf = np.isinf(got) & (np.sign(got) == np.sign(ref))
        good = np.where(must_inf, right_inf, np.where(must_fin, inside, inside | right_inf))
        if allow is not None:
            good = good | (fin & np.asarray(allow, dtype=bool) & ~gfin)
        good = np.where(np.isnan(ref), ~gfin, good)
        good = np.where(np.isinf(ref), right_inf | np.isnan(got), good)
        ratio = np.where(fin & gfin & ~must_inf, np.abs(got - np.where(fin, ref, 0.0)) / bnd, 0.0)
    counts = {"must_inf": int(must_inf.sum()), "must_finite": int(must_fin.sum()), "undecided": int(und.sum()),
              "ref_nonfinite": int((~fin).sum())}
    if not good.all():
        return False, math.inf, int(np.argmin(good.ravel())), counts
    i = int(np.argmax(ratio)) if ratio.size else 0
    return True, float(ratio.ravel()[i]) if ratio.size else 0.0, i, counts
