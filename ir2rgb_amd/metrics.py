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
"""
import math

import torch

from . import _lib

__all__ = ["video_metrics", "ssim_reference", "VideoScore", "ssim_bound", "l2_bound", "RANGE_BOUND"]

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
# plain torch
# ---------------------------------------------------------------------------------------------
def _batched(orig_u8, pred_u8, what):
    for t in (orig_u8, pred_u8):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{what}: expected a tensor, got {type(t)}")
        if t.dtype != torch.uint8:
            raise TypeError(f"{what}: expected dtype {torch.uint8}, got {t.dtype}")
    if orig_u8.shape != pred_u8.shape:
        raise ValueError(f"{what}: {tuple(orig_u8.shape)} against {tuple(pred_u8.shape)}")
    if orig_u8.dim() == 3:
        orig_u8, pred_u8 = orig_u8.unsqueeze(0), pred_u8.unsqueeze(0)
    if orig_u8.dim() != 4 or orig_u8.shape[-1] != 3 or orig_u8.shape[0] < 1:
        raise ValueError(f"{what}: uint8 [H,W,3] or [N,H,W,3] expected, got {tuple(pred_u8.shape)}")
    if orig_u8.shape[1] < 7 or orig_u8.shape[2] < 7:
        raise ValueError(f"{what}: the 7x7 window needs H, W >= 7, got {tuple(orig_u8.shape[1:3])}")
    return orig_u8, pred_u8


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


# ---------------------------------------------------------------------------------------------
# the kernels
# ---------------------------------------------------------------------------------------------
_WORKSPACES = {}


def _workspace(device, stream, N, H, W):
    """One fp64 buffer per (device, stream, N, H, W): the library writes all of it before reading, so it is neither
    zeroed nor shared between streams whose launches could overlap."""
    key = (device.index, stream, N, H, W)
    ws = _WORKSPACES.get(key)
    if ws is None:
        nbytes = _lib.lib().ir2rgb_video_metrics_workspace_bytes(N, H, W)
        if nbytes < 0:
            raise ValueError(f"video_metrics: N={N}, H={H}, W={W} is outside what the kernels take "
                             "(N <= 65535, H, W >= 7, 3*H*W < 2**31)")
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
    ws = _workspace(dev, _lib.current_stream(out), N, H, W)
    _lib.launch("ir2rgb_video_metrics_u8", out, orig_u8, pred_u8, given, out, ws, ws.numel() * 8, N, H, W)
    return out


class VideoScore:
    """The movie scores of scripts/ssim_metric.py: ``add(orig_u8, pred_u8)`` appends the per-frame rows of
    ``video_metrics`` on the device, ``result()`` averages them (``ssim_movie`` / ``mse_movie``) and is the only call that
    synchronises."""

    def __init__(self, data_range="reference"):
        self.data_range = data_range
        self._rows = []

    def add(self, orig_u8, pred_u8):
        """One frame [H,W,3] or several [N,H,W,3]; -> their rows [N,3] (device)."""
        rows = video_metrics(orig_u8, pred_u8, self.data_range)
        self._rows.append(rows)
        return rows

    @property
    def frames(self):
        return sum(r.shape[0] for r in self._rows)

    def per_frame(self):
        """fp64 [frames,3] device tensor (ssim, l2, R), in the order added."""
        if not self._rows:
            raise ValueError("VideoScore: no frame was added")
        return torch.cat(self._rows)

    def result(self):
        per = self.per_frame()
        ssim, l2 = per[:, :2].mean(0).tolist()
        return {"ssim": ssim, "l2": l2, "frames": per.shape[0], "per_frame": per}
