"""SSIM and L2 scores of translated frames against a ground-truth RGB track: the reference's evaluation step.

    ssim_single_frame / mse_single_frame / ssim_movie / mse_movie                scripts/ssim_metric.py:16-46

The script converts both uint8 frames with ``skimage.color.rgb2gray``, calls scikit-image's windowed SSIM (7x7 uniform
window, sample covariance, K1 = 0.01, K2 = 0.03) with ``dynamic_range = original_gray.max() - predicted_gray.min()``, takes
``np.linalg.norm(original_gray - predicted_gray)`` as its "mse", and averages both over the movie.  Here that is one entry
point of the kernel library (csrc/video_metrics.hip, fp64 throughout) working on device frames -- the ones
``VideoTranslator`` hands out -- so nothing is copied to the host and nothing synchronises per frame:

* ``video_metrics(orig_u8, pred_u8)``    -> fp64 device tensor [N,3]: ssim, l2, R per frame (the kernels; GPU only)
* ``ssim_reference(orig_u8, pred_u8)``   the same definition in plain torch fp64 on any device (tests, users without a GPU)
* ``VideoScore``                          per-frame rows collected on the device, ``result()`` = the movie averages
* ``ssim_bound`` / ``l2_bound`` / ``RANGE_BOUND``   how far two fp64 evaluations of the definition may lie apart

The definition, per frame (H, W >= 7):

    gray = (r/255)*0.2125 + (g/255)*0.7154 + (b/255)*0.0721           rgb2gray of a uint8 image: img_as_float, then the dot
    R    = max(gray(orig)) - min(gray(pred))                           the script's rule as written, or the value given
    l2   = sqrt(sum (gray(orig) - gray(pred))**2)
    for every 7x7 window inside the image, with the means ux, uy, uxx, uyy, uxy of x, y, x*x, y*y, x*y over its 49 pixels:
        vx = 49/48 (uxx - ux*ux), vy = 49/48 (uyy - uy*uy), vxy = 49/48 (uxy - ux*uy)
        S  = ((2 ux uy + C1)(2 vxy + C2)) / ((ux*ux + uy*uy + C1)(vx + vy + C2)),  C1 = (0.01 R)**2, C2 = (0.03 R)**2
    ssim = mean of S over the (H-6)(W-6) windows

scikit-image filters with reflected borders and crops 3 pixels afterwards: the cropped region never sees a border, so
nothing is padded here.  There are no special cases: R <= 0, flat images and 0/0 behave as IEEE arithmetic does in NumPy,
so an all-black pair scores NaN.

Temporal consistency: the warp error of consecutive frames, the trainer's ``G_Warp`` term as a score
(models/discriminator.py:137-138, ``MaskedL1Loss``, ``Model.resample`` in base_model.py:129-136; csrc/warp_error.hip):

* ``warp_error(prev_u8, cur_u8, flow, weight=None)``   -> fp64 device tensor [N,3]: warp_l1, warp_mse, coverage per pair
* ``warp_error_reference(...)``                          the same definition in plain torch fp64 on any device
* ``warp_bound(H, W, flow, weight)``                     how far two fp64 evaluations of the definition may lie apart, [N,3]
* ``VideoScore.add_pair``                                per-pair rows of a prediction and of the ground truth beside it

A *pair* is two consecutive frames of one track, ``prev`` and ``cur``, uint8 [H,W,3] with H, W >= 2, with a flow ``f``
(fp32 [2,H,W], x then y, in pixels, from ``cur`` to ``prev``) and an optional weight ``m`` (fp32 [1,H,W]; absent means 1).
Everything is in fp64; bytes and fp32 inputs convert exactly.  For pixel (y, x):

    gx = (-1 + x*(2/(W-1))) + fx/((W-1)/2)
    ix = ((gx + 1)*W - 1)*0.5, then clamped to [0, W-1]            likewise iy from y, fy and H

which is ``get_grid`` (an align_corners=True lattice) fed to ``grid_sample(align_corners=False, padding_mode="border")``:
the reference's mismatch, which ``warp_blend`` (csrc/heads.hip) and ``vid2vid.resample`` reproduce too.  It is kept on
purpose: the score is the trainer's G_Warp, not a cleaned-up cousin.  With x0 = floor(ix), x1 = min(x0+1, W-1),
ax = ix - x0, and likewise in y:

    w_c = (1-ay)(1-ax) prev[y0,x0,c] + (1-ay) ax prev[y0,x1,c] + ay (1-ax) prev[y1,x0,c] + ay ax prev[y1,x1,c]
    d_c = cur[y,x,c] - w_c                                           (byte units)
    S1 = sum m |d_c|     S2 = sum m d_c**2     SC = sum m             (S1, S2 over pixels and channels, SC over pixels)

    warp_l1  = S1 / (127.5 * 3 * H * W)     masked_l1(fake_B, resample(fake_B_prev, flow_ref), conf_ref) on the normalised
                                            frames = G_Warp / lambda_T
    warp_mse = S2 / (255**2 * 3 * SC)       masked mean squared error in [0,1] image units (the usual "warping error")
    coverage = SC / (H * W)

There are no special cases: SC = 0 gives 0/0 = NaN as IEEE does; a NaN flow vector or weight stays in the sums of its own
pair (the clamp keeps a NaN, so ax / ay carry it) and leaves every other pair of the batch bit-unchanged; an infinite flow
vector lands on the border like any large one.  No address leaves the frame: indices are clamped as integers, a NaN
coordinate maps to index 0.

Colour: RGB PSNR and the CIELAB error of a frame against its target (csrc/colour_metrics.hip).  Every score above is taken
after ``rgb2gray`` or between consecutive frames: a translator that outputs the right luminance and no colour at all scores
an SSIM of 0.9998 against the 64x128 colour test image of tests/test_colour_metrics_cpu.py while the two lie a mean CIELAB
distance of 63.0 apart (about 2.3 is already visible).

* ``colour_metrics(orig_u8, pred_u8)``    -> fp64 device tensor [N,5]: mse, psnr, delta_e, delta_l, delta_c per frame
* ``colour_reference(orig_u8, pred_u8)``  the same definition in plain torch fp64 on any device
* ``colour_bound(H, W, psnr)``            how far two fp64 evaluations of the definition may lie apart, [5]
* ``srgb_table(device)``                  the 256 doubles both of them read
* ``VideoScore(colour=True)``             collects the rows beside the others

Two uint8 frames ``orig`` and ``pred``, [H,W,3] with H, W >= 1; the constants are scikit-image's ``rgb2lab`` (D65, 2 degree
observer).  Everything is fp64:

    lin[v], v = 0..255:  c = v/255;  lin = c/12.92 if c <= 0.04045 else ((c + 0.055)/1.055)**2.4
        formed once on the host in Python floats (``srgb_table``): kernel and reference read the same 256 doubles
    r, g, b = lin[R], lin[G], lin[B]
    tX = (0.412453 r + 0.357580 g + 0.180423 b) / 0.95047        products and sums left to right, then the division
    tY = (0.212671 r + 0.715160 g + 0.072169 b) / 1.0
    tZ = (0.019334 r + 0.119193 g + 0.950227 b) / 1.08883
    f(t) = cbrt(t) if t > 0.008856 else 7.787 t + 16.0/116.0
    L = 116 f(tY) - 16        a = 500 (f(tX) - f(tY))        b = 200 (f(tY) - f(tZ))

    per pixel, with dL, da, db the differences orig - pred:
        dE = sqrt(dL*dL + da*da + db*db)     (CIE76)
        dC = sqrt(da*da + db*db)             (the distance in the colour plane: what a gray-only score cannot see)
    per frame:
        mse     = (sum over pixels and channels of (orig - pred)**2 in byte units) / (3 H W)
        psnr    = 10 * log10(65025.0 / mse)
        delta_e = sum dE / (H W)        delta_l = sum |dL| / (H W)        delta_c = sum dC / (H W)

There are no special cases: identical frames give ``mse = 0``, ``psnr = +inf`` (65025/0) and exact zeros in the three Lab
columns, and one such frame makes the movie's mean ``psnr`` infinite.  ``mse`` is a sum of integers below 2**53, the same
double in any order; the three Lab sums have a fixed order on the device (bit-reproducible, frames never mix).
"""
import math

import numpy
import torch

from . import _lib

__all__ = ["video_metrics", "ssim_reference", "VideoScore", "ssim_bound", "l2_bound", "RANGE_BOUND",
           "warp_error", "warp_error_reference", "warp_bound",
           "colour_metrics", "colour_reference", "colour_bound", "srgb_table"]

# ---------------------------------------------------------------------------------------------
# The bound between two fp64 evaluations of the definition (written down before any kernel ran).
#
# u = 2**-53 is the unit roundoff: one correctly rounded operation has relative error <= u.
#   gray      three divisions, three products, two additions on values in [0, 1]: every term carries <= 2u, the two
#             additions one u each                                                          -> <= 4u absolute
#   means     six additions along the row, six down the column, one division, on inputs that carry the 4u (8u for the
#             products, plus one u of their own)                                           -> <= 16u for ux, uy and, to first
#             order in the worst case, 22u for uxx, uyy, uxy
#   variances 49/48 (uxx - ux*ux): 22u + 2*16u + 3u of its own operations, times 49/48      -> <= 64u absolute, also vxy
#   S         = (A1 A2) / (B1 B2) with A1 = 2 ux uy + C1, B1 = ux^2 + uy^2 + C1, A2 = 2 vxy + C2, B2 = vx + vy + C2.
#             |A1| <= B1 (2ab <= a^2 + b^2) and |A2| <= B2 (Cauchy-Schwarz) up to those errors; B1 >= C1, B2 >= C2 - 128u.
#             To first order |dS| <= (|dA1| + |dB1|) / B1 + (|dA2| + |dB2|) / B2 + 4u
#                                 <= 2 * 70u / C1 + 2 * 128u / C2 + 4u  <=  256 u (1 + 1/C1 + 1/C2)
#             per window, and a mean of such values carries no more (its own additions: (H-6)(W-6) u relative of a value
#             <= 1 in the worst case, ~1e-10 at 512x1024, inside the first term's slack since 1/C1 >= 1e4).
#   l2        sqrt of a sum of H*W squares <= 1, each with <= 16u, summed in any order       -> <= 64 u sqrt(H*W)
#   R         a difference of two gray values                                               -> <= 8u
# With R >= 0.5 (every test input has a near-white pixel in orig and a near-black one in pred): C1 >= 2.5e-5,
# C2 >= 2.25e-4 and ssim_bound <= 1.3e-9; a wrong window, crop, covariance normalisation, range rule or gray weight moves
# ssim by more than 1e-4 on the same inputs (tests/test_metrics_cpu.py).
# ---------------------------------------------------------------------------------------------
U = 2.0 ** -53
RANGE_BOUND = 8 * U


def ssim_bound(R):
    """Largest difference between two fp64 evaluations of ``ssim`` with data range ``R`` (a float or a tensor)."""
    C1, C2 = (0.01 * R) ** 2, (0.03 * R) ** 2
    return 256 * U * (1 + 1 / C1 + 1 / C2)


def l2_bound(H, W):
    """Largest difference between two fp64 evaluations of ``l2`` on an H x W frame."""
    return 64 * U * math.sqrt(H * W)


# ---------------------------------------------------------------------------------------------
# The bound between two fp64 evaluations of the warp error (written down before the kernel first ran).
#
# Coordinate, one evaluation, with F = |fx| * 2 / (W - 1) (the flow in lattice units; (W - 1) / 2 is exact):
#   a = x * (2/(W-1))   the step and the product round once each, a <= 2                       -> <= 4u
#   b = -1 + a          |b| <= 1                                                                -> <= 5u
#   c = fx / ((W-1)/2)  one division                                                           -> <= u F
#   gx = b + c          |gx| <= 1 + F                                                          -> <= 6u + 2u F
#   e = gx + 1          |e| <= 2 + F                                                           -> <= 8u + 3u F
#   g = e * W                                                                                  -> <= W (10u + 4u F)
#   ix = (g - 1) * 0.5  the halving is exact                                                   -> <= W (6u + 2.5u F)
#                                                                                               = 6u W + 5u |fx| W/(W-1)
#   The clamp does not enlarge it.  A linspace lattice (torch's symmetric evaluation, <= 3u on b) stays inside the same
#   figure.  Two evaluations therefore lie within  Ex = 16u (W + max|fx| W/(W-1))  of each other, Ey likewise with H, fy.
# Warp: w_c is continuous in (ix, iy) -- across integer coordinates, where the neighbour that changes has weight 0, and
#   across the clamp -- and piecewise bilinear between bytes, so its slope is at most 255 per pixel along either axis:
#   |dw| <= 255 (Ex + Ey).  Its own arithmetic (four weights of two factors, four products, three additions on a convex
#   combination of values <= 255; on normalised frames the conversions (v/255 - 0.5)/0.5 and the products a*m, b*m of
#   masked_l1 instead) stays below 32u * 255 per evaluation.  Per channel:
#       D = 255 (Ex + Ey) + 64u * 255                                                          bound on |d_c - d_c'|
# Sums, with A = sum |m| over the pixels and n = 3 H W terms; a sum of n rounded terms taken in ANY order is within
#   (n - 1) u sum|terms| of the exact one, each term m|d| <= 255 |m| (m d^2 <= 255^2 |m|) carries two more roundings:
#       dS1 = 3 A D + (n + 2) u * 3 * 255 A
#       dS2 = 3 A (2 * 255 D + D^2) + (n + 3) u * 3 * 255^2 A
#       dSC = H W u A
# Columns (one division each; r = A / |SC| is 1 for weights >= 0, so that S2 / (255^2 * 3 |SC|) <= r):
#       warp_l1   (dS1 + u * 3 * 255 A) / (127.5 * 3 H W)
#       warp_mse  dS2 / (255^2 * 3 |SC|) + r dSC / |SC| + 3u r
#       coverage  (dSC + u A) / (H W)
# At 512x1024 with a flow of a few pixels: Ex ~ 2e-12, D ~ 1e-9 bytes, and the sums' (n u ~ 1.7e-10 relative) term leads;
# at 16x32 the coordinate term leads at ~1e-13 relative.  A wrong align_corners, padding, flow order or sign, a dropped
# mask or the warp applied to the wrong frame moves the sums by more than 6e-5 relative (tests/test_warp_error_cpu.py).
# A non-finite flow or weight makes the bound non-finite too: such rows are compared as NaN patterns, not by distance.
# ---------------------------------------------------------------------------------------------
def warp_bound(H, W, flow, weight=None):
    """Largest difference between two fp64 evaluations of ``warp_error`` on these inputs: fp64 [N,3] for the columns
    warp_l1, warp_mse, coverage.  ``flow`` [N,2,H,W] (or [2,H,W]), ``weight`` [N,1,H,W] (or [1,H,W]) or None."""
    flow = flow.unsqueeze(0) if flow.dim() == 3 else flow
    N = flow.shape[0]
    f = flow.to(torch.float64).abs().reshape(N, 2, -1).amax(-1)
    if weight is None:
        A = SC = torch.full((N,), float(H * W), dtype=torch.float64, device=flow.device)
    else:
        m = weight.to(torch.float64).reshape(N, -1)
        A, SC = m.abs().sum(-1), m.sum(-1).abs()
    Ex, Ey = 16 * U * (W + f[:, 0] * W / (W - 1)), 16 * U * (H + f[:, 1] * H / (H - 1))
    D = 255 * (Ex + Ey) + 64 * U * 255
    n = 3 * H * W
    dS1 = 3 * A * D + (n + 2) * U * 3 * 255 * A
    dS2 = 3 * A * (2 * 255 * D + D * D) + (n + 3) * U * 3 * 255 ** 2 * A
    dSC = H * W * U * A
    r = A / SC
    return torch.stack([(dS1 + U * 3 * 255 * A) / (127.5 * n), dS2 / (255 ** 2 * 3 * SC) + r * dSC / SC + 3 * U * r,
                        (dSC + U * A) / (H * W)], 1)


# ---------------------------------------------------------------------------------------------
# The bound between two fp64 evaluations of the colour scores (written down before the kernel first ran).
#
#   lin       both evaluations read the same 256 doubles                                      -> 0
#   t         three products, two sums, one division on values with t <= 1.0001               -> <= 6u relative
#   f         cube-root branch: the 6u of t arrive divided by 3 (2u), the library's cbrt adds E_cbrt = 2u -- ASSUMED for
#             either side: the device library documents <= 1 ulp for its fp64 cbrt and so does glibc for the one behind
#             numpy.cbrt, f <= 1.0001; nobody has measured either.  Should a GPU test disagree, that is a finding: E_cbrt is
#             then widened to a documented figure, never fitted to the observed error -- plus one u of slack
#                                                                                             -> <= 5u absolute
#             linear branch: 7.787 * 6u * 0.008856, one product, one sum                      -> <= 2u absolute
#             No colour sits near the branch: over all 2**24 colours and the three rows the smallest |t - 0.008856| is
#             2.24e-9, nine orders above 6u (tests/test_colour_metrics_cpu.py repeats the sweep)
#   Lab       L = 116 f - 16: 116 * 5u + its own two roundings on values <= 116              -> |dL| <= 800u
#             a = 500 (fX - fY): 500 * 10u + the roundings of a difference <= 1 and a product <= 500   -> <= 2**13 u
#             b = 200 (fY - fZ)                                                               -> <= 2**12 u
#             per frame; twice that for the difference of two frames' values
#   pixel     dE, |dL| and dC are 1-Lipschitz in (dL, da, db): the vector moves by <= 2 (800 + 2**13 + 2**12) u < 2**15 u
#             less their own roundings (three squares, two sums, one correctly rounded sqrt on values <= 300: <= 4 * 300u),
#             inside the same figure                                                          -> E_px = 2**15 u
#   mean      H W terms <= 300 summed in any order and divided once                           -> (H W + 1) * 300u
#   columns 2-4: 2**15 u + (H W + 1) * 300u       1.7e-8 at 512x1024, 2.1e-11 at 16x32
#   mse       exact                                                                           -> 0
#   psnr      one division (u relative in the argument = u / ln 10 absolute in log10), log10 at <= 2 ulp of a value <= 15,
#             one product by 10                                                               -> 8u + 4u |psnr|
#             an infinite psnr (identical frames) is compared as a pattern, not by distance
# A skipped gamma, a white point of (1,1,1), channels read as BGR, a dropped linear branch, |d chroma| for dC or means over
# 3 H W move a Lab column by more than 1e-3 (tests/test_colour_metrics_cpu.py).
# ---------------------------------------------------------------------------------------------
E_CBRT = 2 * U


def colour_bound(H, W, psnr=None):
    """Largest difference between two fp64 evaluations of ``colour_metrics`` on an H x W frame: fp64 [5] for the columns
    mse, psnr, delta_e, delta_l, delta_c.  ``psnr``: the frame's value (a float or a one-element tensor); None takes the
    largest finite one a frame of this size can have, ``10 log10(65025 * 3 H W)`` (one byte off by one)."""
    p = 10.0 * math.log10(65025.0 * 3 * H * W) if psnr is None else abs(float(psnr))
    lab = 2.0 ** 15 * U + (H * W + 1) * 300 * U
    return torch.tensor([0.0, 8 * U + 4 * U * p, lab, lab, lab], dtype=torch.float64)


# ---------------------------------------------------------------------------------------------
# plain torch
# ---------------------------------------------------------------------------------------------
def _frames(a, b, what, dtype_text, needs, min_side):
    """The opening check of two uint8 frame batches -> both as [N,H,W,3] and whether they came as one frame [H,W,3];
    anything else raises.  ``dtype_text`` and ``needs`` are the caller's words for the dtype and the smallest side."""
    for t in (a, b):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{what}: expected a tensor, got {type(t)}")
        if t.dtype != torch.uint8:
            raise TypeError(f"{what}: {dtype_text.format(torch.uint8)}, got {t.dtype}")
    if a.shape != b.shape:
        raise ValueError(f"{what}: {tuple(a.shape)} against {tuple(b.shape)}")
    single = a.dim() == 3
    if single:
        a, b = a.unsqueeze(0), b.unsqueeze(0)
    if a.dim() != 4 or a.shape[-1] != 3 or a.shape[0] < 1:
        raise ValueError(f"{what}: uint8 [H,W,3] or [N,H,W,3] expected, got {tuple(b.shape)}")
    if a.shape[1] < min_side or a.shape[2] < min_side:
        raise ValueError(f"{what}: {needs} needs H, W >= {min_side}, got {tuple(a.shape[1:3])}")
    return a, b, single


def _batched(orig_u8, pred_u8, what):
    return _frames(orig_u8, pred_u8, what, "expected dtype {}", "the 7x7 window", 7)[:2]


def _range(data_range, N, device):
    """-> None (the script's rule) or an fp64 [N] tensor on ``device``."""
    if isinstance(data_range, str):
        if data_range != "reference":
            raise ValueError("data_range: 'reference', a number or an fp64 tensor")
        return None
    if isinstance(data_range, torch.Tensor):
        r = data_range.to(device=device, dtype=torch.float64).reshape(-1)
        if r.numel() not in (1, N):
            raise ValueError(f"data_range: one value or one per frame ({N}) expected, got {r.numel()}")
        return r.expand(N).contiguous()
    return torch.full((N,), float(data_range), dtype=torch.float64, device=device)


def _gray(img_u8):
    f = img_u8.to(torch.float64) / 255.0
    return f[..., 0] * 0.2125 + f[..., 1] * 0.7154 + f[..., 2] * 0.0721


def _window_sums(a):
    """[H,W] -> [H-6,W-6]: 7 along the row (left to right), then 7 down the column (top to bottom)."""
    H, W = a.shape
    s = a[:, 0:W - 6]
    for k in range(1, 7):
        s = s + a[:, k:W - 6 + k]
    t = s[0:H - 6]
    for k in range(1, 7):
        t = t + s[k:H - 6 + k]
    return t


def ssim_reference(orig_u8, pred_u8, data_range="reference"):
    """``video_metrics`` in plain torch fp64 on whatever device the frames are on: uint8 [H,W,3] or [N,H,W,3] ->
    fp64 [N,3] (ssim, l2, R).  Written from the formulas of this module's docstring in the operation order of
    csrc/video_metrics.hip; the two differ only in the order of the sums over a frame (``ssim_bound``, ``l2_bound``)."""
    orig_u8, pred_u8 = _batched(orig_u8, pred_u8, "ssim_reference")
    N = orig_u8.shape[0]
    given = _range(data_range, N, orig_u8.device)
    rows = []
    for n in range(N):
        x, y = _gray(orig_u8[n]), _gray(pred_u8[n])
        R = given[n] if given is not None else x.max() - y.min()
        d = x - y
        l2 = (d * d).sum().sqrt()
        ux, uy, uxx, uyy, uxy = (_window_sums(a) / 49.0 for a in (x, y, x * x, y * y, x * y))
        cov_norm = 49.0 / 48.0
        vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
        C1, C2 = (0.01 * R) * (0.01 * R), (0.03 * R) * (0.03 * R)
        S = ((2.0 * ux * uy + C1) * (2.0 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
        rows.append(torch.stack([S.mean(), l2, R]))
    return torch.stack(rows)


def _pairs(prev_u8, cur_u8, flow, weight, what):
    """-> prev, cur uint8 [N,H,W,3], flow fp32 [N,2,H,W], weight fp32 [N,1,H,W] or None; anything else raises."""
    for t, name in ((flow, "flow"), (weight, "weight")):
        if t is None and name == "weight":
            continue
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{what}: {name}: expected a tensor, got {type(t)}")
        if t.dtype != torch.float32:
            raise TypeError(f"{what}: {name} of dtype {torch.float32} expected, got {t.dtype}")
    prev_u8, cur_u8, single = _frames(prev_u8, cur_u8, what, "frames of dtype {} expected", "the lattice", 2)
    if single:
        if flow.dim() != 3 or (weight is not None and weight.dim() != 3):
            raise ValueError(f"{what}: one pair takes flow [2,H,W] and weight [1,H,W]")
        flow, weight = flow.unsqueeze(0), weight.unsqueeze(0) if weight is not None else None
    N, H, W = prev_u8.shape[:3]
    if tuple(flow.shape) != (N, 2, H, W):
        raise ValueError(f"{what}: flow {tuple(flow.shape)} given, {(N, 2, H, W)} expected")
    if weight is not None and tuple(weight.shape) != (N, 1, H, W):
        raise ValueError(f"{what}: weight {tuple(weight.shape)} given, {(N, 1, H, W)} expected")
    return prev_u8, cur_u8, flow, weight


def _axis(idx, f, n):
    """One axis of the warp: lattice positions ``idx``, flow component ``f`` in pixels, size ``n`` -> (weight of the second
    neighbour, first index, second index).  A NaN coordinate keeps its NaN in the weight and reads index 0."""
    g = (-1.0 + idx * (2.0 / (n - 1))) + f / ((n - 1) / 2.0)
    p = ((g + 1.0) * n - 1.0) * 0.5
    p = p.clamp(0.0, float(n - 1))                  # (torch's clamp keeps a NaN)
    fl = p.floor()
    i0 = torch.nan_to_num(fl, nan=0.0).long().clamp(0, n - 1)
    return p - fl, i0, (i0 + 1).clamp(max=n - 1)


def warp_error_reference(prev_u8, cur_u8, flow, weight=None):
    """``warp_error`` in plain torch fp64 on whatever device the tensors are on -> fp64 [N,3] (warp_l1, warp_mse,
    coverage).  Written from the formulas of this module's docstring in the operation order of csrc/warp_error.hip; the two
    differ only in the order of the sums over a pair (``warp_bound``)."""
    prev_u8, cur_u8, flow, weight = _pairs(prev_u8, cur_u8, flow, weight, "warp_error_reference")
    N, H, W = prev_u8.shape[:3]
    f64, dev = torch.float64, prev_u8.device
    xs, ys = torch.arange(W, dtype=f64, device=dev).view(1, W), torch.arange(H, dtype=f64, device=dev).view(H, 1)
    rows = []
    for n in range(N):
        P, C = prev_u8[n].to(f64), cur_u8[n].to(f64)
        ax, x0, x1 = _axis(xs, flow[n, 0].to(f64), W)
        ay, y0, y1 = _axis(ys, flow[n, 1].to(f64), H)
        w00, w01, w10, w11 = (1.0 - ay) * (1.0 - ax), (1.0 - ay) * ax, ay * (1.0 - ax), ay * ax
        wv = (w00.unsqueeze(-1) * P[y0, x0] + w01.unsqueeze(-1) * P[y0, x1] + w10.unsqueeze(-1) * P[y1, x0]
              + w11.unsqueeze(-1) * P[y1, x1])
        d = C - wv
        m = weight[n, 0].to(f64).unsqueeze(-1) if weight is not None else torch.ones((H, W, 1), dtype=f64, device=dev)
        S1, S2, SC = (m * d.abs()).sum(), (m * (d * d)).sum(), m.sum()
        rows.append(torch.stack([S1 / (127.5 * 3 * H * W), S2 / (255.0 * 255.0 * 3.0 * SC), SC / (H * W)]))
    return torch.stack(rows)


_LIN = {}


def srgb_table(device=None):
    """fp64 [256]: the sRGB decoding of a byte, ``c = v/255; c/12.92 if c <= 0.04045 else ((c + 0.055)/1.055)**2.4``, in
    Python floats (``math.pow``) on the host, as a tensor on ``device`` (default: the CPU).  One tensor per device, made at
    the first call and never modified: ``colour_metrics`` and ``colour_reference`` read the same 256 doubles."""
    device = torch.device("cpu" if device is None else device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    t = _LIN.get(device)
    if t is None:
        c = [v / 255 for v in range(256)]
        lin = [x / 12.92 if x <= 0.04045 else math.pow((x + 0.055) / 1.055, 2.4) for x in c]
        t = _LIN[device] = torch.tensor(lin, dtype=torch.float64).to(device)
    return t


def _cbrt(t):
    return torch.from_numpy(numpy.cbrt(t.cpu().numpy())).to(t.device)


def _lab(img_u8):
    """uint8 [...,3] -> (L, a, b), fp64 [...] each, in the operation order of csrc/colour_metrics.hip."""
    v = srgb_table(img_u8.device)[img_u8.long()]
    r, g, b = v[..., 0], v[..., 1], v[..., 2]
    tx = (0.412453 * r + 0.357580 * g + 0.180423 * b) / 0.95047
    ty = (0.212671 * r + 0.715160 * g + 0.072169 * b) / 1.0
    tz = (0.019334 * r + 0.119193 * g + 0.950227 * b) / 1.08883
    fx, fy, fz = (torch.where(t > 0.008856, _cbrt(t), 7.787 * t + 16.0 / 116.0) for t in (tx, ty, tz))
    return 116.0 * fy - 16.0, 500.0 * (fx - fy), 200.0 * (fy - fz)


def colour_reference(orig_u8, pred_u8):
    """``colour_metrics`` in plain torch fp64 on whatever device the frames are on: uint8 [H,W,3] or [N,H,W,3] -> fp64
    [N,5] (mse, psnr, delta_e, delta_l, delta_c).  Written from the formulas of this module's docstring in the operation
    order of csrc/colour_metrics.hip; the two differ in the order of the three Lab sums and in the cube root
    (``colour_bound``).  The cube root is ``numpy.cbrt`` on a CPU copy of ``t`` -- the C library's ``cbrt``, documented
    within 1 ulp -- and not ``torch.pow(t, 1/3)``, which is a ``pow`` with a rounded exponent and carries no such claim."""
    orig_u8, pred_u8, _ = _frames(orig_u8, pred_u8, "colour_reference", "expected dtype {}", "a frame", 1)
    N, H, W = orig_u8.shape[:3]
    rows = []
    for n in range(N):
        d = orig_u8[n].to(torch.float64) - pred_u8[n].to(torch.float64)
        mse = (d * d).sum() / (3 * H * W)
        (Lo, ao, bo), (Lp, ap, bp) = _lab(orig_u8[n]), _lab(pred_u8[n])
        dL, da, db = Lo - Lp, ao - ap, bo - bp
        dE, dC = (dL * dL + da * da + db * db).sqrt(), (da * da + db * db).sqrt()
        peak = mse.new_tensor(65025.0)          # (a number / a tensor is reciprocal() * number in torch: two roundings)
        rows.append(torch.stack([mse, 10.0 * torch.log10(peak / mse), dE.sum() / (H * W), dL.abs().sum() / (H * W),
                                 dC.sum() / (H * W)]))
    return torch.stack(rows)


# ---------------------------------------------------------------------------------------------
# the kernels
# ---------------------------------------------------------------------------------------------
_WORKSPACES = {}


def _workspace(entry, limits, device, stream, N, H, W):
    """One fp64 buffer per (entry, device, stream, N, H, W), sized by ``ir2rgb_<entry>_workspace_bytes``: the library
    writes all of it before reading, so it is neither zeroed nor shared between streams whose launches could overlap."""
    key = (entry, device.index, stream, N, H, W)
    ws = _WORKSPACES.get(key)
    if ws is None:
        nbytes = getattr(_lib.lib(), f"ir2rgb_{entry}_workspace_bytes")(N, H, W)
        if nbytes < 0:
            raise ValueError(f"{entry}: N={N}, H={H}, W={W} is outside what the kernels take ({limits})")
        ws = _WORKSPACES[key] = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=device)
    return ws


def tile():
    """(rows, columns) of SSIM windows one workgroup evaluates (``ir2rgb_video_metrics_tile``; host only)."""
    lib = _lib.lib()
    return lib.ir2rgb_video_metrics_tile(0), lib.ir2rgb_video_metrics_tile(1)


def video_metrics(orig_u8, pred_u8, data_range="reference"):
    """Scores of ``pred_u8`` against the ground truth ``orig_u8``: uint8 [H,W,3] or [N,H,W,3] device tensors ->
    fp64 device tensor [N,3] with the columns ssim, l2, R (``ir2rgb_video_metrics_u8``).  Enqueued on the current
    stream; nothing synchronises the host.

    ``data_range``: ``"reference"`` (default) is the script's rule as written, per frame
    ``R = gray(orig).max() - gray(pred).min()``, formed on the device.  A number or an fp64 tensor (one value, or one per
    frame) is used instead of it.  scikit-image releases differ in what they do with the script's ``dynamic_range=``
    keyword: those that honour it compute what ``"reference"`` computes; those that silently drop it fall back on the
    range of the dtype, which for the float64 images ``rgb2gray`` returns is ``2.0`` (-1 .. 1) -- pass ``2.0`` to
    reproduce such a release.  ``1.0`` is the conventional range of a gray image in [0, 1].

    CPU tensors, other dtypes, non-contiguous tensors and frames smaller than the 7x7 window raise."""
    dev = _lib.require_device(orig_u8, pred_u8, dtype=torch.uint8)
    orig_u8, pred_u8 = _batched(orig_u8, pred_u8, "video_metrics")
    N, H, W = orig_u8.shape[:3]
    given = _range(data_range, N, dev)
    out = torch.empty((N, 3), dtype=torch.float64, device=dev)
    ws = _workspace("video_metrics", "N <= 65535, H, W >= 7, 3*H*W < 2**31", dev, _lib.current_stream(out), N, H, W)
    _lib.launch("ir2rgb_video_metrics_u8", out, orig_u8, pred_u8, given, out, ws, ws.numel() * 8, N, H, W)
    return out


def warp_error(prev_u8, cur_u8, flow, weight=None):
    """Warp error of ``cur_u8`` against ``prev_u8`` warped along ``flow``: uint8 [H,W,3] or [N,H,W,3] device frames, fp32
    ``flow`` [2,H,W] / [N,2,H,W] (x then y, in pixels, from ``cur`` to ``prev``) and an optional fp32 ``weight`` [1,H,W] /
    [N,1,H,W] (the confidence of the flow; None means 1) -> fp64 device tensor [N,3] with the columns warp_l1, warp_mse,
    coverage (``ir2rgb_warp_error_u8``; the definition is in this module's docstring).  Enqueued on the current stream;
    nothing synchronises the host.

    CPU tensors, other dtypes, non-contiguous tensors and frames smaller than 2x2 raise."""
    dev = _lib.require_device(prev_u8, cur_u8, dtype=torch.uint8)
    if _lib.require_device(flow, weight, dtype=torch.float32) != dev:
        raise ValueError("warp_error: frames and flow on different devices")
    prev_u8, cur_u8, flow, weight = _pairs(prev_u8, cur_u8, flow, weight, "warp_error")
    N, H, W = prev_u8.shape[:3]
    out = torch.empty((N, 3), dtype=torch.float64, device=dev)
    ws = _workspace("warp_error", "N <= 65535, H, W >= 2, 3*H*W < 2**31", dev, _lib.current_stream(out), N, H, W)
    _lib.launch("ir2rgb_warp_error_u8", out, prev_u8, cur_u8, flow, weight, out, ws, ws.numel() * 8, N, H, W)
    return out


def colour_metrics(orig_u8, pred_u8):
    """Colour scores of ``pred_u8`` against the ground truth ``orig_u8``: uint8 [H,W,3] or [N,H,W,3] device tensors -> fp64
    device tensor [N,5] with the columns mse, psnr, delta_e, delta_l, delta_c (``ir2rgb_colour_metrics_u8``; the definition
    is in this module's docstring).  Enqueued on the current stream; nothing synchronises the host (the device's
    ``srgb_table`` is copied once, at the first call).

    CPU tensors, other dtypes and non-contiguous tensors raise."""
    dev = _lib.require_device(orig_u8, pred_u8, dtype=torch.uint8)
    orig_u8, pred_u8, _ = _frames(orig_u8, pred_u8, "colour_metrics", "expected dtype {}", "a frame", 1)
    N, H, W = orig_u8.shape[:3]
    out = torch.empty((N, 5), dtype=torch.float64, device=dev)
    ws = _workspace("colour_metrics", "N <= 65535, H, W >= 1, 3*H*W < 2**31", dev, _lib.current_stream(out), N, H, W)
    _lib.launch("ir2rgb_colour_metrics_u8", out, orig_u8, pred_u8, srgb_table(dev), out, ws, ws.numel() * 8, N, H, W)
    return out


class VideoScore:
    """The movie scores of scripts/ssim_metric.py: ``add(orig_u8, pred_u8)`` appends the per-frame rows of
    ``video_metrics`` on the device, ``result()`` averages them (``ssim_movie`` / ``mse_movie``) and is the only call that
    synchronises.  ``add_pair`` collects the temporal rows (``warp_error`` of the prediction, and of the ground truth as the
    baseline: how much of the error is the flow's own); ``result()`` reports them only when a pair was added.  With
    ``colour=True`` every ``add`` also appends the rows of ``colour_metrics``; ``result()`` then reports their column means
    too (one pair of identical frames makes the movie's ``psnr`` infinite).  Without it nothing more is launched."""

    def __init__(self, data_range="reference", colour=False):
        self.data_range = data_range
        self.colour = bool(colour)
        self._rows = []
        self._pair_rows = []
        self._colour_rows = []

    def add(self, orig_u8, pred_u8):
        """One frame [H,W,3] or several [N,H,W,3]; -> their rows [N,3] (device)."""
        rows = video_metrics(orig_u8, pred_u8, self.data_range)
        self._rows.append(rows)
        if self.colour:
            self._colour_rows.append(colour_metrics(orig_u8, pred_u8))
        return rows

    @property
    def frames(self):
        return sum(r.shape[0] for r in self._rows)

    def per_frame(self):
        """fp64 [frames,3] device tensor (ssim, l2, R), in the order added."""
        if not self._rows:
            raise ValueError("VideoScore: no frame was added")
        return torch.cat(self._rows)

    def add_pair(self, pred_prev_u8, pred_cur_u8, orig_prev_u8, orig_cur_u8, flow, weight=None):
        """Two consecutive outputs and their ground-truth frames with the flow (and its confidence) between the latter;
        -> rows [N,5] (device): warp_l1, warp_mse of the prediction, the same of the ground truth, coverage."""
        pred = warp_error(pred_prev_u8, pred_cur_u8, flow, weight)
        orig = warp_error(orig_prev_u8, orig_cur_u8, flow, weight)
        rows = torch.cat([pred[:, :2], orig[:, :2], pred[:, 2:]], 1)
        self._pair_rows.append(rows)
        return rows

    @property
    def pairs(self):
        return sum(r.shape[0] for r in self._pair_rows)

    def per_pair(self):
        """fp64 [pairs,5] device tensor (warp_l1, warp_mse, truth_warp_l1, truth_warp_mse, coverage), in the order added."""
        if not self._pair_rows:
            raise ValueError("VideoScore: no pair was added")
        return torch.cat(self._pair_rows)

    def per_frame_colour(self):
        """fp64 [frames,5] device tensor (mse, psnr, delta_e, delta_l, delta_c), in the order added."""
        if not self._colour_rows:
            raise ValueError("VideoScore: no colour row was added (VideoScore(colour=True))")
        return torch.cat(self._colour_rows)

    def result(self):
        per = self.per_frame()
        ssim, l2 = per[:, :2].mean(0).tolist()
        res = {"ssim": ssim, "l2": l2, "frames": per.shape[0], "per_frame": per}
        if self._pair_rows:
            pp = self.per_pair()
            res.update(zip(("warp_l1", "warp_mse", "truth_warp_l1", "truth_warp_mse", "coverage"), pp.mean(0).tolist()))
            res.update(pairs=pp.shape[0], per_pair=pp)
        if self._colour_rows:
            pc = self.per_frame_colour()
            res.update(zip(("mse", "psnr", "delta_e", "delta_l", "delta_c"), pc.mean(0).tolist()))
            res.update(per_frame_colour=pc)
        return res
