"""CPU side of the video scores (ir2rgb_amd.metrics, csrc/video_metrics.hip): the plain-torch restatement
``ssim_reference`` -- what tests/test_metrics_gpu.py holds the kernels to -- against an independent formulation that composes
``scipy.ndimage.uniform_filter`` exactly as scikit-image's ``compare_ssim`` does, the bound of ``ssim_bound`` against
injected faults, the entry points in every table, argument validation before any launch, and the host logic of
``VideoTranslator.evaluate``.  The inputs and shapes defined here are the ones the GPU file uses."""
import functools
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("random", "smooth", "flat", "identical")
NAMES = ("ir2rgb_video_metrics_workspace_bytes", "ir2rgb_video_metrics_tile", "ir2rgb_video_metrics_u8")
BT601 = (0.299, 0.587, 0.114)


# ---------------------------------------------------------------------------------------------
# shapes and inputs (imported by tests/test_metrics_gpu.py)
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def tile():
    from ir2rgb_amd import _lib, build, metrics
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return metrics.tile()


def small_shapes():
    """One window, one more in either direction, a ragged shape; exactly one tile, one pixel more and one less in both
    directions; several tiles."""
    TR, TC = tile()
    return [(7, 7), (7, 8), (8, 7), (9, 13), (TR + 6, TC + 6), (TR + 7, TC + 7), (TR + 5, TC + 5), (64, 128)]


FULL = (512, 1024)


def make_pair(kind, H, W, seed):
    """uint8 [H,W,3] ground truth and prediction with R >= 0.5 by construction: one near-white pixel in ``orig``, one
    near-black pixel in ``pred``."""
    g = torch.Generator().manual_seed(seed)
    noise = lambda: torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8)
    if kind == "random":
        orig, pred = noise(), noise()
    elif kind == "smooth":      # a gradient, and the same gradient with a little noise: high SSIM
        ramp = 40 + 160 * (torch.arange(H).view(H, 1, 1) / max(H - 1, 1) + torch.arange(W).view(1, W, 1) / max(W - 1, 1)) / 2
        ramp = ramp + torch.tensor([0.0, 10.0, -10.0])
        orig = ramp.round().to(torch.uint8)
        pred = (ramp + torch.randint(-6, 7, (H, W, 3), generator=g)).round().clamp(0, 255).to(torch.uint8)
    elif kind == "flat":        # variance 0 on one side
        orig, pred = torch.full((H, W, 3), 128, dtype=torch.uint8), noise()
    elif kind == "identical":
        orig = noise()
        orig[-1, -1] = 3
        pred = orig
    else:
        raise ValueError(kind)
    orig, pred = orig.clone(), pred.clone()
    orig[0, 0] = 250
    pred[-1, -1] = 3
    if kind == "identical":
        pred[0, 0] = 250
    return orig.contiguous(), pred.contiguous()


@functools.lru_cache(None)
def reference(kind, H, W, seed, data_range="reference"):
    """(orig, pred, fp64 [3] row of ssim_reference), computed once per process and never modified."""
    from ir2rgb_amd import metrics
    orig, pred = make_pair(kind, H, W, seed)
    return orig, pred, metrics.ssim_reference(orig, pred, data_range)[0]


def assert_rows_close(got, want, H, W, what=""):
    """``got``, ``want``: fp64 [3] (ssim, l2, R) within ssim_bound / l2_bound / RANGE_BOUND; NaN only where both are."""
    from ir2rgb_amd import metrics
    got, want = [float(v) for v in got], [float(v) for v in want]
    bounds = (metrics.ssim_bound(want[2]), metrics.l2_bound(H, W), metrics.RANGE_BOUND)
    print(what, (H, W), "differences", [abs(a - b) for a, b in zip(got, want)], "bounds", bounds)
    for name, a, b, tol in zip(("ssim", "l2", "R"), got, want, bounds):
        if np.isnan(b):
            assert np.isnan(a), (what, name, a, b)
        else:
            assert abs(a - b) <= tol, (what, (H, W), name, a, b, abs(a - b), tol)


# ---------------------------------------------------------------------------------------------
# the independent formulation: scikit-image's composition of scipy's filter
# ---------------------------------------------------------------------------------------------
def skimage_formulation(orig, pred, data_range="reference", win=7, sample_cov=True, crop=None, swapped_range=False,
                        weights=(0.2125, 0.7154, 0.0721)):
    """rgb2gray + compare_ssim(gaussian_weights=False) + np.linalg.norm as scikit-image spells them: uniform_filter with
    its default reflected border on the whole image, the S map, then a crop of (win - 1) // 2.  The keyword arguments
    inject the faults the bound has to reject."""
    ndimage = pytest.importorskip("scipy.ndimage")
    X = (orig.numpy().astype(np.float64) / 255) @ np.array(weights)
    Y = (pred.numpy().astype(np.float64) / 255) @ np.array(weights)
    if data_range == "reference":
        R = Y.max() - X.min() if swapped_range else X.max() - Y.min()
    else:
        R = float(data_range)
    NP = win ** 2
    cov_norm = NP / (NP - 1) if sample_cov else 1.0
    f = lambda a: ndimage.uniform_filter(a, size=win)
    ux, uy, uxx, uyy, uxy = f(X), f(Y), f(X * X), f(Y * Y), f(X * Y)
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    C1, C2 = (0.01 * R) ** 2, (0.03 * R) ** 2
    A1, A2, B1, B2 = 2 * ux * uy + C1, 2 * vxy + C2, ux ** 2 + uy ** 2 + C1, vx + vy + C2
    with np.errstate(invalid="ignore", divide="ignore"):
        S = (A1 * A2) / (B1 * B2)
    pad = (win - 1) // 2 if crop is None else crop
    S = S[pad:S.shape[0] - pad, pad:S.shape[1] - pad]
    return np.array([S.mean(), np.linalg.norm(X - Y), R])


@pytest.mark.parametrize("kind", KINDS)
def test_reference_agrees_with_the_skimage_composition_at_every_gpu_shape(kind):
    for i, (H, W) in enumerate(small_shapes() + [FULL]):
        orig, pred, want = reference(kind, H, W, 100 + i)
        assert float(want[2]) >= 0.5
        assert_rows_close(want, skimage_formulation(orig, pred), H, W, f"{kind} vs scipy")


def test_reference_with_a_given_range_and_a_batch():
    from ir2rgb_amd import metrics
    pairs = [make_pair(k, 40, 52, 7 + i) for i, k in enumerate(("random", "smooth", "flat"))]
    O, P = torch.stack([p[0] for p in pairs]), torch.stack([p[1] for p in pairs])
    rng = torch.tensor([0.75, 1.0, 2.0], dtype=torch.float64)
    rows = metrics.ssim_reference(O, P, rng)
    assert rows.shape == (3, 3) and rows.dtype == torch.float64 and torch.equal(rows[:, 2], rng)
    for n in range(3):
        assert_rows_close(rows[n], skimage_formulation(O[n], P[n], float(rng[n])), 40, 52, "given range")
        assert torch.equal(rows[n], metrics.ssim_reference(O[n], P[n], float(rng[n]))[0])       # frames never mix
    one = metrics.ssim_reference(O, P, 1.0)
    assert torch.equal(one[:, 2], torch.ones(3, dtype=torch.float64)) and torch.equal(one[:, 1], rows[:, 1])
    assert not torch.equal(one[:, 0], metrics.ssim_reference(O, P)[:, 0])


FAULTS = {"window 6": dict(win=6), "window 8": dict(win=8), "no 49/48": dict(sample_cov=False), "crop 2": dict(crop=2),
          "crop 4": dict(crop=4), "R from pred.max - orig.min": dict(swapped_range=True), "BT.601 gray": dict(weights=BT601)}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_the_bound_rejects_injected_faults(fault):
    """Every plausible mistake moves ssim by more than 1000 x the bound the GPU test allows (on the non-trivial inputs:
    a pair of identical images scores 1 whatever the window or the constants are)."""
    from ir2rgb_amd import metrics
    TR, TC = tile()
    for kind in ("random", "smooth", "flat"):
        for i, (H, W) in enumerate([(TR + 7, TC + 7), (64, 128)]):
            orig, pred = make_pair(kind, H, W, 300 + i)
            good, bad = skimage_formulation(orig, pred), skimage_formulation(orig, pred, **FAULTS[fault])
            moved, bound = abs(good[0] - bad[0]), metrics.ssim_bound(good[2])
            print(fault, kind, (H, W), "moves ssim by", moved, "bound", bound)
            assert moved > 1000 * bound, (fault, kind, (H, W), moved, bound)


def test_bound_values():
    from ir2rgb_amd import metrics
    u = 2.0 ** -53
    assert metrics.ssim_bound(0.5) == 256 * u * (1 + 1 / 0.005 ** 2 + 1 / 0.015 ** 2) and 1.2e-9 < metrics.ssim_bound(0.5) < 1.3e-9
    assert metrics.ssim_bound(1.0) < metrics.ssim_bound(0.5)
    assert metrics.l2_bound(512, 1024) == 64 * u * np.sqrt(512 * 1024) and metrics.RANGE_BOUND == 8 * u


def test_identical_and_all_black_pairs():
    from ir2rgb_amd import metrics
    for H, W in ((7, 7), (9, 13), (64, 128)):
        orig, pred, row = reference("identical", H, W, 5)
        assert torch.equal(orig, pred)
        assert abs(float(row[0]) - 1.0) <= metrics.ssim_bound(float(row[2])) and float(row[1]) == 0.0
    black = torch.zeros(12, 9, 3, dtype=torch.uint8)
    row = metrics.ssim_reference(black, black)[0]
    assert np.isnan(float(row[0])) and float(row[1]) == 0.0 and float(row[2]) == 0.0
    assert np.isnan(skimage_formulation(black, black)[0])


def test_reference_refuses_what_the_kernels_refuse():
    from ir2rgb_amd import metrics
    a = torch.zeros(8, 8, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="7x7 window"):
        metrics.ssim_reference(a[:6], a[:6])
    with pytest.raises(TypeError, match="uint8"):
        metrics.ssim_reference(a.float(), a.float())
    with pytest.raises(ValueError):
        metrics.ssim_reference(a, a[:7])
    with pytest.raises(ValueError, match="data_range"):
        metrics.ssim_reference(a, a, "skimage")


# ---------------------------------------------------------------------------------------------
# the entry points are declared, bound, wrapped and validate their arguments
# ---------------------------------------------------------------------------------------------
def test_entry_points_are_present_everywhere():
    import ir2rgb_amd
    from ir2rgb_amd import _lib, fastbind, metrics
    header = open(os.path.join(ROOT, "include", "ir2rgb_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for n, ret in zip(NAMES, ("long", "int", "int")):
        assert re.search(r"\b%s\s+%s\s*\(" % (ret, n), header)
        assert n in _lib.PROTOTYPES and n in fastbind.wrappable()
    tile()
    lib = _lib.lib()
    for n in NAMES:
        assert getattr(lib, n) is getattr(lib.fast_module, n)
    assert os.path.exists(os.path.join(ROOT, "ir2rgb_amd", "csrc", "video_metrics.hip"))
    assert ir2rgb_amd.video_metrics is metrics.video_metrics and ir2rgb_amd.VideoScore is metrics.VideoScore
    assert ir2rgb_amd.ssim_reference is metrics.ssim_reference


def test_workspace_and_tile_queries():
    from ir2rgb_amd import _lib
    TR, TC = tile()
    lib = _lib.lib()
    assert TR > 0 and TC > 0 and lib.ir2rgb_video_metrics_tile(2) == -1
    ws = lib.ir2rgb_video_metrics_workspace_bytes
    for H, W in small_shapes() + [FULL]:
        sizes = [ws(N, H, W) for N in (1, 2, 3, 8)]
        assert sizes[0] > 0 and sizes[0] % 8 == 0 and all(b > a for a, b in zip(sizes, sizes[1:]))
    assert ws(1, 512, 1024) > ws(1, 64, 128) > ws(1, 7, 7)
    for bad in ((0, 64, 64), (1, 6, 64), (1, 64, 6), (-1, 64, 64), (70000, 64, 64), (1, 32768, 32768)):
        assert ws(*bad) < 0


def test_bad_arguments_are_refused_before_any_launch():
    from ir2rgb_amd import _lib
    tile()
    lib = _lib.lib()
    buf = torch.zeros(1 << 16, dtype=torch.float64)     # host memory: nothing may be launched on it
    p = buf.data_ptr()
    assert p % 8 == 0
    need = lib.ir2rgb_video_metrics_workspace_bytes(2, 16, 20)
    ok = (p, p, None, p, p, need, 2, 16, 20, None)

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[("orig", "pred", "range", "out", "ws", "bytes", "N", "H", "W", "stream").index(k)] = v
        return lib.ir2rgb_video_metrics_u8(*a)

    for k in ("orig", "pred", "out", "ws"):
        assert call(**{k: None}) == -1
    assert call(N=0) == -1 and call(H=6) == -1 and call(W=6) == -1 and call(bytes=need - 8) == -1 and call(bytes=0) == -1
    assert call(out=p + 4) == -3 and call(range=p + 4) == -3 and call(ws=p + 2) == -3
    assert lib.ctypes_handle.ir2rgb_video_metrics_u8(p, p, None, p + 4, p, need, 2, 16, 20, None) == -3     # ctypes agrees


def test_cpu_tensors_and_bad_inputs_raise():
    from ir2rgb_amd import metrics
    a = torch.zeros(8, 8, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="no CPU fallback"):
        metrics.video_metrics(a, a)
    with pytest.raises(ValueError, match="no CPU fallback"):
        metrics.VideoScore().add(a, a)
    with pytest.raises(TypeError):
        metrics.video_metrics(a.numpy(), a.numpy())
    with pytest.raises(ValueError, match="no frame"):
        metrics.VideoScore().result()


# ---------------------------------------------------------------------------------------------
# VideoTranslator.evaluate: which target an output is scored against
# ---------------------------------------------------------------------------------------------
def test_outputs_are_scored_against_the_target_of_their_input_frame():
    from ir2rgb_amd.inference import SequenceState, VideoTranslator
    assert callable(VideoTranslator.evaluate)
    for tG in (2, 3, 5):
        s = SequenceState(tG)
        produced = [i for i in range(tG + 6) if s.push()]          # input frames that complete a window
        assert produced[0] == tG - 1
        assert [s.output_frame(k) for k in range(len(produced))] == produced
        s.reset()
        assert s.output_frame(0) == tG - 1
