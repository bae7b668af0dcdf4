"""CPU side of the colour scores (ir2rgb_amd.metrics.colour_metrics, csrc/colour_metrics.hip): the plain-torch restatement
``colour_reference`` -- what tests/test_colour_metrics_gpu.py holds the kernels to -- against published CIELAB values and
against an independent formulation (matrix form, its own sRGB decoding, ``t ** (1/3)``, sums taken column by column), the
bound of ``colour_bound`` against planted faults, the sweep of all 2**24 colours past the branch threshold of ``f``, what the
gray-only scores cannot see, the entry points in every table, argument validation before any launch, ``VideoScore`` with and
without colour, and the host logic of ``VideoTranslator.evaluate(colour=True)``.  The inputs and shapes defined here are the
ones the GPU file uses."""
import functools
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ir2rgb_colour_metrics_workspace_bytes", "ir2rgb_colour_metrics_u8")
KINDS = ("random", "dark", "grey")
# the smallest sizes and single rows / columns; ragged ones (one-pixel form); the wide form below one workgroup; exactly one
# 1024-pixel partial row, just under and just over; several workgroups
SHAPES = [(1, 1), (1, 5), (3, 1), (7, 13), (17, 33), (16, 32), (32, 32), (33, 31), (32, 36), (64, 128)]
FULL = (512, 1024)          # 512 partial-row candidates, more than the 256 cap: the grid-stride loop
FAULT_SHAPES = [s for s in SHAPES if s[0] >= 7] + [FULL]
COLUMNS = ("mse", "psnr", "delta_e", "delta_l", "delta_c")
U = 2.0 ** -53


# ---------------------------------------------------------------------------------------------
# inputs (imported by tests/test_colour_metrics_gpu.py)
# ---------------------------------------------------------------------------------------------
def built():
    from ir2rgb_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.lib()


def colour_image(H, W):
    """uint8 [H,W,3]: saturated colours, the hue running along x (and a little along y), the value rising with y."""
    y, x = torch.arange(H, dtype=torch.float64).view(H, 1), torch.arange(W, dtype=torch.float64).view(1, W)
    h = (x / W + 0.13 * y / H) % 1.0
    s = 0.75 + 0.25 * torch.cos(0.9 * y + 0.4 * x)
    v = 0.45 + 0.55 * (y + 1) / H
    chans = []
    for n in (5.0, 3.0, 1.0):                                   # the usual closed form of HSV -> RGB
        k = (n + h * 6.0) % 6.0
        chans.append(v - v * s * torch.minimum(torch.minimum(k, 4.0 - k), torch.ones_like(k)).clamp(min=0.0))
    return (torch.stack(chans, -1) * 255.0).round().clamp(0, 255).to(torch.uint8).contiguous()


def grey_copy(img_u8):
    """``rgb2gray`` of the image, rounded to bytes and written back into three channels."""
    f = img_u8.double()
    g = (f[..., 0] * 0.2125 + f[..., 1] * 0.7154 + f[..., 2] * 0.0721).round().clamp(0, 255).to(torch.uint8)
    return g.unsqueeze(-1).expand(-1, -1, 3).contiguous()


def make_pair(kind, H, W, seed=None):
    """uint8 [H,W,3] orig and pred.  ``random``: bytes.  ``dark``: bytes // 16, so that the linear branch of ``f`` carries
    most pixels.  ``grey``: a colour image against its own gray copy."""
    g = torch.Generator().manual_seed(1000 * H + W if seed is None else seed)
    if kind == "grey":
        img = colour_image(H, W)
        return img, grey_copy(img)
    a = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8)
    b = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8)
    if kind == "dark":
        return a // 16, b // 16
    if kind != "random":
        raise ValueError(kind)
    return a, b


@functools.lru_cache(None)
def reference(kind, H, W):
    """(orig, pred, fp64 [5] row of colour_reference, fp64 [5] bound): computed once per process and never modified."""
    from ir2rgb_amd import metrics
    orig, pred = make_pair(kind, H, W)
    want = metrics.colour_reference(orig, pred)[0]
    return orig, pred, want, metrics.colour_bound(H, W, want[1])


def assert_rows_close(got, want, bound, what=""):
    """fp64 [5] rows: mse bit-equal, psnr and the Lab columns within their bounds; an infinite value only where both are."""
    got, want, bound = got.tolist(), want.tolist(), bound.tolist()
    print(what, "differences", [abs(a - b) if math.isfinite(b) else (a, b) for a, b in zip(got, want)], "bounds", bound)
    assert got[0] == want[0], (what, "mse", got[0], want[0])
    for name, a, b, tol in zip(COLUMNS[1:], got[1:], want[1:], bound[1:]):
        if not math.isfinite(b):
            assert a == b, (what, name, a, b)
        else:
            assert abs(a - b) <= tol, (what, name, a, b, abs(a - b), tol)


M_XYZ = ((0.412453, 0.357580, 0.180423), (0.212671, 0.715160, 0.072169), (0.019334, 0.119193, 0.950227))
WHITE = (0.95047, 1.0, 1.08883)


def formulation(orig, pred, gamma=True, white=WHITE, bgr=False, linear_branch=True, chroma_diff=False, per_channel=False):
    """The five columns written another way: its own sRGB decoding (torch.pow), the XYZ conversion as a matrix product,
    ``t ** (1/3)`` for the cube root, sums column by column, NumPy's log10.  The keyword arguments plant the faults the
    bound has to reject."""
    H, W = orig.shape[:2]

    def lab(img):
        c = img.double() / 255.0
        if bgr:
            c = c.flip(-1)
        lin = torch.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4) if gamma else c
        t = (lin.reshape(-1, 3) @ torch.tensor(M_XYZ, dtype=torch.float64).t()).reshape(H, W, 3)
        t = t / torch.tensor(white, dtype=torch.float64)
        root = t ** (1.0 / 3.0)
        f = torch.where(t > 0.008856, root, 7.787 * t + 16.0 / 116.0) if linear_branch else root
        return torch.stack([116.0 * f[..., 1] - 16.0, 500.0 * (f[..., 0] - f[..., 1]), 200.0 * (f[..., 1] - f[..., 2])], -1)

    lo, lp = lab(orig), lab(pred)
    d = lo - lp
    dE = d.pow(2).sum(-1).sqrt()
    dC = (lo[..., 1:].norm(dim=-1) - lp[..., 1:].norm(dim=-1)).abs() if chroma_diff else d[..., 1:].pow(2).sum(-1).sqrt()
    count = H * W * (3 if per_channel else 1)
    mse = float(((orig.double() - pred.double()) ** 2).mean())
    with np.errstate(divide="ignore"):
        psnr = float(10.0 * np.log10(np.float64(65025.0) / np.float64(mse)))
    cols = [t.sum(0).sum() / count for t in (dE, d[..., 0].abs(), dC)]
    return torch.stack([torch.tensor(mse, dtype=torch.float64), torch.tensor(psnr, dtype=torch.float64)] + cols)


# ---------------------------------------------------------------------------------------------
# the definition
# ---------------------------------------------------------------------------------------------
def test_lab_of_the_primaries_matches_published_values():
    from ir2rgb_amd import metrics
    table = {(255, 255, 255): (100.0, 0.0, 0.0), (0, 0, 0): (0.0, 0.0, 0.0), (255, 0, 0): (53.24, 80.09, 67.20),
             (0, 255, 0): (87.73, -86.18, 83.18), (0, 0, 255): (32.30, 79.19, -107.86), (128, 128, 128): (53.585, 0.0, 0.0)}
    L, a, b = metrics._lab(torch.tensor(list(table), dtype=torch.uint8))
    for i, (rgb, want) in enumerate(table.items()):
        got = (float(L[i]), float(a[i]), float(b[i]))
        print(rgb, got, want)
        for x, w in zip(got, want):
            assert abs(x - w) <= 1e-2, (rgb, got, want)


def test_srgb_table():
    from ir2rgb_amd import metrics
    lin = metrics.srgb_table()
    assert lin.dtype == torch.float64 and lin.shape == (256,) and lin.device.type == "cpu"
    assert metrics.srgb_table() is lin and metrics.srgb_table("cpu") is lin         # one tensor per device
    c = np.arange(256, dtype=np.float64) / 255.0
    want = np.where(c <= 0.04045, c / 12.92, np.power((c + 0.055) / 1.055, 2.4))
    got = lin.numpy()
    assert bool((np.abs(got - want) <= np.spacing(want)).all())                     # 1 ulp
    assert bool((np.diff(got) > 0).all())
    assert got[0] == 0.0 and got[255] == 1.0
    assert got[10] == 10 / 255 / 12.92 and got[11] == math.pow((11 / 255 + 0.055) / 1.055, 2.4)     # either side of 0.04045


@pytest.mark.parametrize("kind", KINDS)
def test_reference_agrees_with_an_independent_formulation_at_every_gpu_shape(kind):
    for H, W in SHAPES + ([FULL] if kind == "random" else []):
        orig, pred, want, bound = reference(kind, H, W)
        assert want.dtype == torch.float64 and want.shape == (5,)
        assert_rows_close(formulation(orig, pred), want, bound, f"{kind} {(H, W)} vs matrix form")


def test_no_colour_sits_within_rounding_of_the_branch_threshold():
    """Two evaluations of f could take different branches if some colour's t lay within their rounding (6u) of 0.008856:
    the smallest distance over all 2**24 colours and the three rows, in the kernel's operation order."""
    from ir2rgb_amd import metrics
    lin = metrics.srgb_table().numpy()
    smallest = math.inf
    for (cr, cg, cb), w in zip(M_XYZ, WHITE):
        rg = (cr * lin)[:, None] + (cg * lin)[None, :]                              # [R,G]
        for B in range(256):
            t = (rg + cb * lin[B]) / w
            smallest = min(smallest, float(np.abs(t - 0.008856).min()))
    print("smallest |t - 0.008856| over all colours and rows:", smallest)
    assert smallest >= 1e-12


def test_a_grey_copy_scores_as_perfect_in_ssim_and_far_off_in_colour():
    from ir2rgb_amd import metrics
    for H, W in ((16, 32), (64, 128)):
        orig, pred, want, _ = reference("grey", H, W)
        ssim = float(metrics.ssim_reference(orig, pred)[0, 0])
        print((H, W), "ssim", ssim, "row", want.tolist())
        assert ssim > 0.99 and float(want[4]) > 30.0
        assert float(want[4]) <= float(want[2]) and float(want[3]) <= float(want[2])    # dC, |dL| <= dE pixel by pixel


FAULTS = {"gamma skipped": dict(gamma=False), "white point (1,1,1)": dict(white=(1.0, 1.0, 1.0)),
          "channels read as BGR": dict(bgr=True), "linear branch dropped": dict(linear_branch=False),
          "dC as the difference of chroma": dict(chroma_diff=True), "means over 3 H W": dict(per_channel=True)}


@functools.lru_cache(None)
def _good(kind, H, W):
    orig, pred = reference(kind, H, W)[:2]
    return formulation(orig, pred)


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_the_bound_rejects_planted_faults(fault):
    """Every plausible mistake moves one of the three Lab columns by more than 1000 x the bound the GPU test allows, on
    random and on dark pairs at every shape from (7,13) up, the full frame included, and by more than 1e-3 at every listed
    shape.  The full frame is not asked for the absolute figure: orig and pred are drawn alike, so a fault that treats both
    the same way (swapped channels) moves a mean over H W independent pixels by a deviation that shrinks as 1/sqrt(H W) --
    9.8e-4 on the dark 512x1024 pair, still 5e4 x its bound."""
    for kind in ("random", "dark"):
        for H, W in FAULT_SHAPES:
            orig, pred, _, bound = reference(kind, H, W)
            moved = (_good(kind, H, W) - formulation(orig, pred, **FAULTS[fault])).abs()[2:]
            print(fault, kind, (H, W), "moves delta_e, delta_l, delta_c by", moved.tolist(), "bound", float(bound[2]))
            assert bool((moved > 1000 * bound[2:]).any()), (fault, kind, (H, W), moved.tolist(), bound.tolist())
            assert (H, W) == FULL or float(moved.max()) > 1e-3, (fault, kind, (H, W), moved.tolist())


# ---------------------------------------------------------------------------------------------
# fixed rows
# ---------------------------------------------------------------------------------------------
def test_identical_frames_score_zero_and_infinite_psnr():
    from ir2rgb_amd import metrics
    for kind, (H, W) in (("random", (7, 13)), ("dark", (16, 32)), ("grey", (1, 1))):
        orig = reference(kind, H, W)[0]
        row = metrics.colour_reference(orig, orig.clone())[0].tolist()
        assert row == [0.0, math.inf, 0.0, 0.0, 0.0], row


def test_mse_is_exact():
    from ir2rgb_amd import metrics
    for kind in KINDS:
        for H, W in SHAPES + [FULL]:
            if (H, W) == FULL and kind != "random":
                continue
            orig, pred, want, _ = reference(kind, H, W)
            sse = int(((orig.long() - pred.long()) ** 2).sum())
            assert float(want[0]) == sse / (3 * H * W)
            assert float(want[1]) == float(10.0 * torch.log10(torch.tensor(65025.0, dtype=torch.float64) / want[0]))
    one = torch.zeros(2, 2, 3, dtype=torch.uint8)
    other = one.clone()
    other[0, 0, 0] = 1
    assert float(metrics.colour_reference(one, other)[0, 0]) == 1 / 12


def batch(H=7, W=13):
    """Three frame pairs of one size: random, dark, the gray copy."""
    pairs = [make_pair(kind, H, W, seed=80 + i) for i, kind in enumerate(KINDS)]
    return torch.stack([p[0] for p in pairs]), torch.stack([p[1] for p in pairs])


def test_reference_rows_are_per_frame():
    from ir2rgb_amd import metrics
    O, P = batch()
    rows = metrics.colour_reference(O, P)
    assert rows.shape == (3, 5) and rows.dtype == torch.float64
    for n in range(3):
        assert torch.equal(rows[n], metrics.colour_reference(O[n], P[n])[0])
    assert not torch.equal(rows[0], rows[1])


def test_bound_values():
    """The five columns at a shape worked by hand from the comment block in metrics.py."""
    from ir2rgb_amd import metrics
    b = metrics.colour_bound(16, 32, 30.0)
    assert b.shape == (5,) and b.dtype == torch.float64
    lab = (32768 + 513 * 300) * U                       # 2**15 u + (16 * 32 + 1) * 300 u = 186668 u
    assert b.tolist() == [0.0, 128 * U, lab, lab, lab] and abs(lab - 2.07e-11) < 1e-13
    assert metrics.colour_bound(16, 32, torch.tensor(-30.0, dtype=torch.float64)).tolist() == b.tolist()
    full = metrics.colour_bound(512, 1024, 8.0)
    assert float(full[1]) == 40 * U and 1.7e-8 < float(full[2]) < 1.8e-8
    widest = metrics.colour_bound(16, 32)               # no psnr given: the largest finite one of the size
    assert float(widest[1]) == 8 * U + 4 * U * 10.0 * math.log10(65025.0 * 3 * 16 * 32) and widest[2:].tolist() == [lab] * 3
    assert metrics.colour_bound(16, 32, math.inf)[1] == math.inf
    assert metrics.E_CBRT == 2 * U


# ---------------------------------------------------------------------------------------------
# validation
# ---------------------------------------------------------------------------------------------
def test_reference_refuses_what_the_kernels_refuse():
    from ir2rgb_amd import metrics
    a = torch.zeros(4, 6, 3, dtype=torch.uint8)
    assert metrics.colour_reference(a, a).shape == (1, 5) and metrics.colour_reference(a[:1, :1], a[:1, :1]).shape == (1, 5)
    with pytest.raises(TypeError, match="uint8"):
        metrics.colour_reference(a.float(), a.float())
    with pytest.raises(TypeError):
        metrics.colour_reference(a.numpy(), a.numpy())
    with pytest.raises(ValueError):
        metrics.colour_reference(a, a[:3])
    with pytest.raises(ValueError):
        metrics.colour_reference(torch.zeros(4, 6, 4, dtype=torch.uint8), torch.zeros(4, 6, 4, dtype=torch.uint8))
    with pytest.raises(ValueError, match="H, W >= 1"):
        metrics.colour_reference(a[:0], a[:0])


def test_cpu_tensors_raise_before_any_launch():
    from ir2rgb_amd import metrics
    a = torch.zeros(8, 8, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="no CPU fallback"):
        metrics.colour_metrics(a, a)
    with pytest.raises(TypeError):
        metrics.colour_metrics(a.numpy(), a.numpy())
    with pytest.raises(ValueError, match="no colour row"):
        metrics.VideoScore(colour=True).per_frame_colour()


def test_entry_points_are_present_everywhere():
    import ir2rgb_amd
    from ir2rgb_amd import _lib, fastbind, metrics
    header = open(os.path.join(ROOT, "include", "ir2rgb_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for n, ret in zip(NAMES, ("long", "int")):
        assert re.search(r"\b%s\s+%s\s*\(" % (ret, n), header)
        assert n in _lib.PROTOTYPES and n in fastbind.wrappable()
    lib = built()
    for n in NAMES:
        assert getattr(lib, n) is getattr(lib.fast_module, n)
    assert os.path.exists(os.path.join(ROOT, "ir2rgb_amd", "csrc", "colour_metrics.hip"))
    for name in ("colour_metrics", "colour_reference", "colour_bound", "srgb_table"):
        assert getattr(ir2rgb_amd, name) is getattr(metrics, name) and name in ir2rgb_amd.__all__ and name in metrics.__all__
    from oracle import window
    assert window.entry_class(NAMES[0]) == "query" and window.entry_class(NAMES[1]) == "op"


def test_workspace_query():
    ws = built().ir2rgb_colour_metrics_workspace_bytes
    for H, W in SHAPES + [FULL, (1024, 1024)]:
        rows = min((H * W + 1023) // 1024, 256)
        assert [ws(N, H, W) for N in (1, 2, 3, 8)] == [32 * rows * N for N in (1, 2, 3, 8)]
    assert ws(1, 1, 1) == 32 and ws(1, 32, 32) == 32 and ws(1, 33, 31) == 32 and ws(1, 32, 36) == 64
    assert ws(1, 512, 1024) == 32 * 256 and ws(65535, 1, 1) == 32 * 65535
    # the sizes tests/test_warp_error_cpu.py lists as bad, with its two one-pixel sides (fine here: H, W >= 1) at zero
    for bad in ((0, 64, 64), (1, 0, 64), (1, 64, 0), (-1, 64, 64), (65536, 64, 64), (1, 32768, 32768)):
        assert ws(*bad) == -1


def test_bad_arguments_are_refused_before_any_launch():
    lib = built()
    buf = torch.zeros(1 << 16, dtype=torch.float64)     # host memory: nothing may be launched on it
    p = buf.data_ptr()
    assert p % 16 == 0
    need = lib.ir2rgb_colour_metrics_workspace_bytes(2, 16, 20)
    ok = (p, p, p, p, p, need, 2, 16, 20, None)
    names = ("orig", "pred", "lin", "out", "ws", "bytes", "N", "H", "W", "stream")

    def call(fn=lib.ir2rgb_colour_metrics_u8, **kw):
        a = list(ok)
        for k, v in kw.items():
            a[names.index(k)] = v
        return fn(*a)

    for k in ("orig", "pred", "lin", "out", "ws"):
        assert call(**{k: None}) == -1
    assert call(N=0) == -1 and call(N=65536) == -1 and call(H=0) == -1 and call(W=0) == -1 and call(H=-3) == -1
    assert call(H=32768, W=32768, bytes=1 << 40) == -1                                      # 3 H W >= 2**31
    assert call(bytes=need - 8) == -1 and call(bytes=0) == -1
    assert call(out=p + 4) == -3 and call(ws=p + 2) == -3 and call(lin=p + 4) == -3 and call(lin=p + 1) == -3
    raw = lib.ctypes_handle.ir2rgb_colour_metrics_u8
    assert call(fn=raw, out=p + 4) == -3 and call(fn=raw, ws=None) == -1 and call(fn=raw, lin=None) == -1


# ---------------------------------------------------------------------------------------------
# VideoScore and VideoTranslator.evaluate: host logic
# ---------------------------------------------------------------------------------------------
TODAY = ["ssim", "l2", "frames", "per_frame"]
PAIR_KEYS = ["warp_l1", "warp_mse", "truth_warp_l1", "truth_warp_mse", "coverage", "pairs", "per_pair"]
COLOUR_KEYS = ["mse", "psnr", "delta_e", "delta_l", "delta_c", "per_frame_colour"]


def test_videoscore_keys_with_and_without_colour():
    from ir2rgb_amd import metrics
    s = metrics.VideoScore()
    assert s.colour is False and s.data_range == "reference"
    s._rows.append(torch.tensor([[0.5, 2.0, 1.0], [0.7, 4.0, 1.0]], dtype=torch.float64))
    assert list(s.result()) == TODAY
    s._pair_rows.append(torch.tensor([[1.0, 2.0, 3.0, 4.0, 0.5], [3.0, 4.0, 5.0, 6.0, 1.0]], dtype=torch.float64))
    assert list(s.result()) == TODAY + PAIR_KEYS
    rows = torch.tensor([[2.0, 40.0, 3.0, 1.0, 2.5], [4.0, 30.0, 5.0, 2.0, 4.5]], dtype=torch.float64)
    s._colour_rows.append(rows[:1]), s._colour_rows.append(rows[1:])
    res = s.result()
    assert list(res) == TODAY + PAIR_KEYS + COLOUR_KEYS
    assert [res[k] for k in COLUMNS] == [3.0, 35.0, 4.0, 1.5, 3.5] == rows.mean(0).tolist()
    assert torch.equal(res["per_frame_colour"], rows) and torch.equal(s.per_frame_colour(), rows)
    assert res["ssim"] == 0.6 and res["warp_l1"] == 2.0
    t = metrics.VideoScore("reference", True)
    assert t.colour is True
    t._rows.append(s._rows[0]), t._colour_rows.append(rows)
    assert list(t.result()) == TODAY + COLOUR_KEYS
    rows[0, 1] = math.inf                                   # one identical pair: the movie's psnr is infinite, stated as such
    assert t.result()["psnr"] == math.inf and t.result()["delta_e"] == 4.0


def test_evaluate_scores_output_k_against_its_target_in_colour(monkeypatch):
    """``evaluate(colour=True)`` without a GPU: the translator's frame loop and the kernels' entry points are replaced by
    their plain-torch restatements; what is checked is which frames are scored against which."""
    from ir2rgb_amd import metrics
    from ir2rgb_amd.inference import SequenceState, VideoTranslator
    tG, H, W, n_in = 3, 8, 12, 7
    g = torch.Generator().manual_seed(6)
    targets = list(torch.randint(0, 256, (n_in, H, W, 3), generator=g, dtype=torch.uint8))
    outs = list(torch.randint(0, 256, (n_in - (tG - 1), H, W, 3), generator=g, dtype=torch.uint8))
    colour_calls = []

    def colour(o, p):
        colour_calls.append((o, p))
        return metrics.colour_reference(o, p)

    monkeypatch.setattr(metrics, "video_metrics", lambda o, p, r="reference": metrics.ssim_reference(o, p, r))
    monkeypatch.setattr(metrics, "colour_metrics", colour)
    tr = VideoTranslator.__new__(VideoTranslator)
    tr.seq = SequenceState(tG)
    tr.translate = lambda frames, real_rgb=None: iter(outs)
    tr._rgb_frame = lambda frame, what: frame
    plain = tr.evaluate(None, targets).result()
    assert list(plain) == TODAY and not colour_calls                        # off: nothing more is called
    assert list(tr.evaluate(None, targets, colour=False).result()) == TODAY and not colour_calls
    res = tr.evaluate(None, targets, colour=True).result()
    assert list(res) == TODAY + COLOUR_KEYS and len(colour_calls) == len(outs)
    assert torch.equal(res["per_frame"], plain["per_frame"]) and res["ssim"] == plain["ssim"] and res["l2"] == plain["l2"]
    pc = res["per_frame_colour"]
    assert pc.shape == (len(outs), 5) and pc.dtype == torch.float64
    for k in range(len(outs)):
        assert torch.equal(pc[k], metrics.colour_reference(targets[tG - 1 + k], outs[k])[0])
        assert not torch.equal(pc[k], metrics.colour_reference(targets[k], outs[k])[0])
    assert [res[c] for c in COLUMNS] == pc.mean(0).tolist()
