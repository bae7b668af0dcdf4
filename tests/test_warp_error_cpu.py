"""CPU side of the temporal consistency score (ir2rgb_amd.metrics.warp_error, csrc/warp_error.hip): the plain-torch
restatement ``warp_error_reference`` -- what tests/test_warp_error_gpu.py holds the kernels to -- against an independent
formulation made of the statements of ``vid2vid.resample`` / ``masked_l1`` on the normalised frames (a linspace lattice,
``F.grid_sample`` in double), the bound of ``warp_bound`` against planted faults, non-finite flows and weights, the entry
points in every table, argument validation before any launch, ``VideoScore`` with and without pairs, and the host logic of
``VideoTranslator.evaluate(temporal=...)``.  The inputs and shapes defined here are the ones the GPU file uses."""
import functools
import os
import re

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ir2rgb_warp_error_workspace_bytes", "ir2rgb_warp_error_u8")
KINDS = ("random", "consistent")
WEIGHTS = ("binary", "fractional", "none", "zero")
# the smallest lattice, one more along either axis, a ragged one (scalar form), one and a bit more than one trip of a
# workgroup in the 4-pixel form, several workgroups
SHAPES = [(2, 2), (2, 3), (3, 2), (7, 13), (16, 32), (17, 33), (40, 52), (64, 128)]
FULL = (512, 1024)
FAULT_SHAPES = [s for s in SHAPES if s[0] >= 7] + [FULL]


# ---------------------------------------------------------------------------------------------
# inputs (imported by tests/test_warp_error_gpu.py)
# ---------------------------------------------------------------------------------------------
def built():
    from ir2rgb_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.lib()


def make_flow(H, W, seed):
    """fp32 [2,H,W]: a seeded Gaussian of a few pixels with planted vectors -- zero, integer-valued, one whose sampling
    position is an integer up to rounding on both axes (bilinear weights 0 / 1, where two evaluations may take different
    floors), +2W along x and -2H along y (both clamps), and one pointing out of the frame at each corner (later ones win
    where a tiny frame makes positions coincide)."""
    g = torch.Generator().manual_seed(seed)
    f = torch.randn(2, H, W, generator=g) * 3.0
    # ix = (x + fx) W / (W - 1) - 0.5 is the integer k for fx = (k + 0.5) (W - 1) / W - x
    y, x = (2 * H) // 3, W // 3
    on_x, on_y = (min(x + 1, W - 1) + 0.5) * (W - 1) / W - x, (max(y - 1, 0) + 0.5) * (H - 1) / H - y
    planted = [(y, x, on_x, on_y),
               (H // 2, W // 2, 0.0, 0.0), (H // 2, W // 3, 2.0, -1.0), (H // 3, W // 2, -3.0, 2.0),
               (H // 3, W // 3, 2.0 * W, 0.5), ((2 * H) // 3, (2 * W) // 3, -0.5, -2.0 * H),
               (0, 0, -1.5, -2.5), (0, W - 1, 1.5, -2.5), (H - 1, 0, -1.5, 2.5), (H - 1, W - 1, 1.5, 2.5)]
    for y, x, fx, fy in planted:
        f[0, y, x], f[1, y, x] = fx, fy
    return f.contiguous()


def make_weight(kind, H, W, seed):
    """fp32 [1,H,W] or None: 0/1 at about 70 %, the bilinear resize of such a map (what FlowNet returns when it had to
    resize), absent, all zero."""
    g = torch.Generator().manual_seed(seed + 1)
    if kind == "none":
        return None
    if kind == "zero":
        return torch.zeros(1, H, W)
    if kind == "binary":
        return (torch.rand(1, H, W, generator=g) < 0.7).float()
    if kind == "fractional":
        coarse = (torch.rand(1, 1, H // 2 + 2, W // 2 + 2, generator=g) < 0.7).float()
        return F.interpolate(coarse, size=(H, W), mode="bilinear")[0].contiguous()
    raise ValueError(kind)


def formulation(prev, cur, flow, weight, align_corners=False, padding="border", swap_xy=False, sign=1.0, use_mask=True,
                warp_cur=False, want_warped=False):
    """The three columns from the trainer's statements: normalise both frames, ``vid2vid.resample`` (get_grid's linspace
    lattice + flow / ((size - 1) / 2), ``F.grid_sample(bilinear, border, align_corners=False)``) and ``masked_l1``, all in
    double, rescaled.  The keyword arguments plant the faults the bound has to reject."""
    H, W = prev.shape[:2]
    norm = lambda t: t.permute(2, 0, 1).double().div(255).sub(0.5).div(0.5).unsqueeze(0)     # noqa: E731
    a, b = norm(cur), norm(prev)
    if warp_cur:
        a, b = b, a
    fl = flow.double().unsqueeze(0)
    if swap_xy:
        fl = fl.flip(1)
    fl = sign * fl
    xs = torch.linspace(-1.0, 1.0, W, dtype=torch.float64).view(1, 1, 1, W).expand(1, 1, H, W)
    ys = torch.linspace(-1.0, 1.0, H, dtype=torch.float64).view(1, 1, H, 1).expand(1, 1, H, W)
    grid = torch.cat([xs, ys], 1) + torch.cat([fl[:, 0:1] / ((W - 1.0) / 2.0), fl[:, 1:2] / ((H - 1.0) / 2.0)], 1)
    warped = F.grid_sample(b, grid.permute(0, 2, 3, 1), mode="bilinear", padding_mode=padding, align_corners=align_corners)
    if want_warped:
        return warped
    m = weight.double().unsqueeze(0) if (weight is not None and use_mask) else torch.ones(1, 1, H, W, dtype=torch.float64)
    mm = m.expand(-1, 3, -1, -1)
    l1 = F.l1_loss(a * mm, warped * mm)                                 # = S1 / 127.5 / (3 H W)
    mse = (mm * (a - warped) ** 2).sum() / 4.0 / (3.0 * m.sum())        # (d / 127.5)^2 = 4 d^2 / 255^2
    return torch.stack([l1, mse, m.sum() / (H * W)])


def make_images(kind, H, W, flow, seed):
    """uint8 [H,W,3] prev and cur.  ``random``: bytes.  ``consistent``: prev is a ramp plus a sinusoid texture and cur is
    prev warped along the flow (by the trainer's statements), rounded to bytes: the right score is rounding noise and any
    fault in the wiring is large."""
    g = torch.Generator().manual_seed(seed + 2)
    if kind == "random":
        return (torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8),
                torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8))
    if kind != "consistent":
        raise ValueError(kind)
    y, x = torch.arange(H, dtype=torch.float64).view(H, 1, 1), torch.arange(W, dtype=torch.float64).view(1, W, 1)
    c = torch.arange(3, dtype=torch.float64).view(1, 1, 3)
    img = 40 + 120 * (0.7 * y / (H - 1) + 0.3 * x / (W - 1)) + 35 * torch.sin(0.9 * x + 0.6 * c) * torch.cos(0.7 * y - 0.4 * c)
    prev = img.round().clamp(0, 255).to(torch.uint8)
    warped = formulation(prev, prev, flow, None, want_warped=True)[0].permute(1, 2, 0)
    cur = ((warped * 0.5 + 0.5) * 255).round().clamp(0, 255).to(torch.uint8)
    return prev.contiguous(), cur.contiguous()


@functools.lru_cache(None)
def reference(kind, wkind, H, W):
    """(prev, cur, flow, weight, fp64 [3] row of warp_error_reference, fp64 [3] bound): computed once per process and
    never modified."""
    from ir2rgb_amd import metrics
    seed = 1000 * H + W
    flow = make_flow(H, W, seed)
    weight = make_weight(wkind, H, W, seed)
    prev, cur = make_images(kind, H, W, flow, seed)
    return prev, cur, flow, weight, metrics.warp_error_reference(prev, cur, flow, weight)[0], metrics.warp_bound(H, W, flow, weight)[0]


def assert_rows_close(got, want, bound, what=""):
    """fp64 [3] rows (warp_l1, warp_mse, coverage) within the three bounds; NaN only where both are."""
    got, want, bound = got.tolist(), want.tolist(), bound.tolist()
    print(what, "differences", [abs(a - b) for a, b in zip(got, want)], "bounds", bound)
    for name, a, b, tol in zip(("warp_l1", "warp_mse", "coverage"), got, want, bound):
        if b != b:
            assert a != a, (what, name, a, b)
        else:
            assert abs(a - b) <= tol, (what, name, a, b, abs(a - b), tol)


# ---------------------------------------------------------------------------------------------
# the restatement against the trainer's statements
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wkind", WEIGHTS)
@pytest.mark.parametrize("kind", KINDS)
def test_reference_agrees_with_the_trainers_statements_at_every_gpu_shape(kind, wkind):
    for H, W in SHAPES + ([FULL] if wkind == "binary" else []):
        prev, cur, flow, weight, want, bound = reference(kind, wkind, H, W)
        assert want.dtype == torch.float64 and want.shape == (3,)
        assert_rows_close(want, formulation(prev, cur, flow, weight), bound, f"{kind} {wkind} {(H, W)} vs grid_sample")
        if wkind == "zero":
            assert float(want[0]) == 0.0 and want[1] != want[1] and float(want[2]) == 0.0      # 0/0, as IEEE does
        if wkind == "none":
            assert float(want[2]) == 1.0


def test_consistent_pairs_score_rounding_noise_only():
    for H, W in SHAPES + [FULL]:
        want = reference("consistent", "none", H, W)[4]
        # |d| <= 0.5 byte: warp_l1 <= 0.5 / 127.5, warp_mse <= 0.25 / 255^2
        assert float(want[0]) <= 0.5 / 127.5 + 1e-12 and float(want[1]) <= 0.25 / 255 ** 2 + 1e-12


FAULTS = {"align_corners=True": dict(align_corners=True), "zero padding": dict(padding="zeros"),
          "flow x / y swapped": dict(swap_xy=True), "flow sign": dict(sign=-1.0), "mask ignored": dict(use_mask=False),
          "cur warped instead of prev": dict(warp_cur=True)}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_the_bound_rejects_planted_faults(fault):
    """Every plausible mistake moves warp_l1 or warp_mse by more than 1000 x the bound the GPU test allows, on both kinds
    of image at every shape from (7,13) up.  The three smallest lattices are not asked: at (2,2) without a flow the
    align_corners=True and =False coordinates clamp onto the same pixel with the same weights, so that fault is all but
    invisible there."""
    for kind in KINDS:
        for H, W in FAULT_SHAPES:
            prev, cur, flow, weight, _, bound = reference(kind, "binary", H, W)
            good, bad = formulation(prev, cur, flow, weight), formulation(prev, cur, flow, weight, **FAULTS[fault])
            moved = (good - bad).abs()
            print(fault, kind, (H, W), "moves warp_l1, warp_mse by", moved[:2].tolist(), "bounds", bound[:2].tolist(),
                  "relative", (moved[:2] / good[:2]).tolist())
            assert float(moved[0]) > 1000 * float(bound[0]) or float(moved[1]) > 1000 * float(bound[1]), \
                (fault, kind, (H, W), moved.tolist(), bound.tolist())


def test_bound_values():
    """The three columns at a shape worked by hand from the comment block in metrics.py, and their order of magnitude."""
    from ir2rgb_amd import metrics
    u = 2.0 ** -53
    H, W = 16, 32
    flow = torch.zeros(2, H, W)
    flow[0, 3, 4], flow[1, 5, 6] = -4.0, 2.0
    b = metrics.warp_bound(H, W, flow, None)
    assert b.shape == (1, 3) and b.dtype == torch.float64
    Ex, Ey = 16 * u * (W + 4.0 * W / (W - 1)), 16 * u * (H + 2.0 * H / (H - 1))
    D = 255 * (Ex + Ey) + 64 * u * 255
    A, n = H * W, 3 * H * W
    want = [(3 * A * D + (n + 2) * u * 765 * A + u * 765 * A) / (127.5 * n),
            (3 * A * (510 * D + D * D) + (n + 3) * u * 3 * 255 ** 2 * A) / (255 ** 2 * 3 * A) + H * W * u + 3 * u,
            (H * W * u * A + u * A) / (H * W)]
    for got, w in zip(b[0].tolist(), want):
        assert abs(got - w) <= 1e-9 * w
    assert 1e-14 < float(b[0, 0]) < 1e-11
    full = metrics.warp_bound(512, 1024, torch.zeros(2, 512, 1024), None)[0]
    assert float(full[0]) < 1e-9 and float(full[1]) < 1e-9 and float(full[2]) < 1e-9
    w = torch.zeros(2, 1, H, W)
    w[0, 0, :4] = 1.0
    two = metrics.warp_bound(H, W, torch.stack([flow, flow]), w)
    assert two.shape == (2, 3) and bool(torch.isfinite(two[0]).all()) and not bool(torch.isfinite(two[1, 1]))   # SC = 0


# ---------------------------------------------------------------------------------------------
# batches, non-finite inputs
# ---------------------------------------------------------------------------------------------
def batch(H=7, W=13):
    """Three pairs: random with a 0/1 weight, consistent with a fractional one, random with ones."""
    P, C, Fl, Wt = [], [], [], []
    for i, (kind, wkind) in enumerate((("random", "binary"), ("consistent", "fractional"), ("random", "none"))):
        flow = make_flow(H, W, 50 + i)
        prev, cur = make_images(kind, H, W, flow, 60 + i)
        w = make_weight(wkind, H, W, 70 + i)
        P.append(prev), C.append(cur), Fl.append(flow), Wt.append(w if w is not None else torch.ones(1, H, W))
    return torch.stack(P), torch.stack(C), torch.stack(Fl), torch.stack(Wt)


def test_reference_rows_are_per_pair():
    from ir2rgb_amd import metrics
    P, C, Fl, Wt = batch()
    rows = metrics.warp_error_reference(P, C, Fl, Wt)
    assert rows.shape == (3, 3) and rows.dtype == torch.float64
    for n in range(3):
        assert torch.equal(rows[n], metrics.warp_error_reference(P[n], C[n], Fl[n], Wt[n])[0])
    assert torch.equal(metrics.warp_error_reference(P[2], C[2], Fl[2], None)[0], rows[2])       # absent means 1


def nonfinite_cases():
    """name -> (flow, weight) of the batch with one planted value in pair 1."""
    _, _, Fl, Wt = batch()
    cases = {}
    for name, val in (("nan flow x", float("nan")), ("inf flow x", float("inf")), ("-inf flow x", float("-inf"))):
        f = Fl.clone()
        f[1, 0, 3, 5] = val
        cases[name] = (f, Wt)
    f = Fl.clone()
    f[1, 1, 2, 2] = float("nan")
    cases["nan flow y"] = (f, Wt)
    for name, val in (("nan weight", float("nan")), ("inf weight", float("inf"))):
        w = Wt.clone()
        w[1, 0, 4, 4] = val
        cases[name] = (Fl, w)
    return cases


def check_nonfinite_rows(name, rows, clean, huge):
    """What the definition gives, without special cases, for a batch whose pair 1 holds one non-finite value: pairs 0 and
    2 bit-unchanged; a NaN flow -> NaN warp_l1 and warp_mse, coverage untouched; an infinite flow -> the row of the same
    flow with +-1e30 in its place (the border); a NaN weight -> a NaN row; an infinite weight -> inf/inf."""
    assert torch.equal(rows[0], clean[0]) and torch.equal(rows[2], clean[2]), name
    r = rows[1]
    if name.startswith("nan flow"):
        assert r[0] != r[0] and r[1] != r[1] and torch.equal(r[2], clean[1, 2]), (name, r)
    elif "inf flow" in name:
        assert bool(torch.isfinite(r).all()) and torch.equal(r, huge[name][1]), (name, r)
    elif name == "nan weight":
        assert bool(torch.isnan(r).all()), (name, r)
    else:
        assert not bool(torch.isfinite(r).any()) and r[1] != r[1], (name, r)


def huge_flow_rows(score):
    P, C, Fl, Wt = batch()
    out = {}
    for name, val in (("inf flow x", 1e30), ("-inf flow x", -1e30)):
        f = Fl.clone()
        f[1, 0, 3, 5] = val
        out[name] = score(P, C, f, Wt)
    return out


def test_nonfinite_flow_and_weight_stay_in_their_pair():
    from ir2rgb_amd import metrics
    P, C, Fl, Wt = batch()
    clean = metrics.warp_error_reference(P, C, Fl, Wt)
    huge = huge_flow_rows(metrics.warp_error_reference)
    for name, (f, w) in nonfinite_cases().items():
        check_nonfinite_rows(name, metrics.warp_error_reference(P, C, f, w), clean, huge)
    zero = metrics.warp_error_reference(P, C, Fl, torch.zeros_like(Wt))
    assert bool((zero[:, 0] == 0).all()) and bool(torch.isnan(zero[:, 1]).all()) and bool((zero[:, 2] == 0).all())


# ---------------------------------------------------------------------------------------------
# validation
# ---------------------------------------------------------------------------------------------
def test_reference_refuses_what_the_kernels_refuse():
    from ir2rgb_amd import metrics
    a, f, w = torch.zeros(4, 6, 3, dtype=torch.uint8), torch.zeros(2, 4, 6), torch.zeros(1, 4, 6)
    assert metrics.warp_error_reference(a, a, f, w).shape == (1, 3)
    with pytest.raises(TypeError, match="uint8"):
        metrics.warp_error_reference(a.float(), a.float(), f)
    with pytest.raises(TypeError, match="float32"):
        metrics.warp_error_reference(a, a, f.double())
    with pytest.raises(TypeError, match="float32"):
        metrics.warp_error_reference(a, a, f, w.double())
    with pytest.raises(TypeError):
        metrics.warp_error_reference(a, a, None)
    with pytest.raises(ValueError):
        metrics.warp_error_reference(a, a[:3], f)
    with pytest.raises(ValueError, match="flow"):
        metrics.warp_error_reference(a, a, f[:, :3])
    with pytest.raises(ValueError, match="flow"):
        metrics.warp_error_reference(a, a, f.unsqueeze(0))
    with pytest.raises(ValueError, match="weight"):
        metrics.warp_error_reference(a, a, f, torch.zeros(4, 6)[None, :, :5])
    with pytest.raises(ValueError, match="H, W >= 2"):
        metrics.warp_error_reference(a[:1], a[:1], f[:, :1], w[:, :1])
    with pytest.raises(ValueError):
        metrics.warp_error_reference(torch.zeros(4, 6, 4, dtype=torch.uint8), torch.zeros(4, 6, 4, dtype=torch.uint8), f)


def test_cpu_tensors_raise_before_any_launch():
    from ir2rgb_amd import metrics
    a, f = torch.zeros(8, 8, 3, dtype=torch.uint8), torch.zeros(2, 8, 8)
    with pytest.raises(ValueError, match="no CPU fallback"):
        metrics.warp_error(a, a, f)
    with pytest.raises(ValueError, match="no CPU fallback"):
        metrics.VideoScore().add_pair(a, a, a, a, f)
    with pytest.raises(TypeError):
        metrics.warp_error(a.numpy(), a.numpy(), f)
    with pytest.raises(ValueError, match="no pair"):
        metrics.VideoScore().per_pair()


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
    assert os.path.exists(os.path.join(ROOT, "ir2rgb_amd", "csrc", "warp_error.hip"))
    for name in ("warp_error", "warp_error_reference", "warp_bound"):
        assert getattr(ir2rgb_amd, name) is getattr(metrics, name) and name in ir2rgb_amd.__all__ and name in metrics.__all__


def test_workspace_query():
    ws = built().ir2rgb_warp_error_workspace_bytes
    for H, W in SHAPES + [FULL, (1024, 1024)]:
        sizes = [ws(N, H, W) for N in (1, 2, 3, 8)]
        assert sizes[0] > 0 and sizes[0] % 24 == 0 and sizes[0] <= 24 * 256 and [s // sizes[0] for s in sizes] == [1, 2, 3, 8]
    assert ws(1, 512, 1024) > ws(1, 64, 128) >= ws(1, 2, 2) == 24
    assert ws(65535, 2, 2) == 24 * 65535
    for bad in ((0, 64, 64), (1, 1, 64), (1, 64, 1), (-1, 64, 64), (65536, 64, 64), (1, 32768, 32768)):
        assert ws(*bad) == -1


def test_bad_arguments_are_refused_before_any_launch():
    lib = built()
    buf = torch.zeros(1 << 16, dtype=torch.float64)     # host memory: nothing may be launched on it
    p = buf.data_ptr()
    assert p % 16 == 0
    need = lib.ir2rgb_warp_error_workspace_bytes(2, 16, 20)
    ok = (p, p, p, p, p, p, need, 2, 16, 20, None)
    names = ("prev", "cur", "flow", "weight", "out", "ws", "bytes", "N", "H", "W", "stream")

    def call(fn=lib.ir2rgb_warp_error_u8, **kw):
        a = list(ok)
        for k, v in kw.items():
            a[names.index(k)] = v
        return fn(*a)

    for k in ("prev", "cur", "flow", "out", "ws"):
        assert call(**{k: None}) == -1
    assert call(N=0) == -1 and call(N=65536) == -1 and call(H=1) == -1 and call(W=1) == -1
    assert call(bytes=need - 8) == -1 and call(bytes=0) == -1
    assert call(out=p + 4) == -3 and call(ws=p + 2) == -3 and call(flow=p + 2) == -3 and call(weight=p + 1) == -3
    assert call(fn=lib.ctypes_handle.ir2rgb_warp_error_u8, out=p + 4) == -3 and call(fn=lib.ctypes_handle.ir2rgb_warp_error_u8, ws=None) == -1


# ---------------------------------------------------------------------------------------------
# VideoScore and VideoTranslator.evaluate: host logic
# ---------------------------------------------------------------------------------------------
def test_videoscore_result_has_todays_keys_without_pairs():
    from ir2rgb_amd import metrics
    s = metrics.VideoScore()
    s._rows.append(torch.tensor([[0.5, 2.0, 1.0], [0.7, 4.0, 1.0]], dtype=torch.float64))
    res = s.result()
    assert list(res) == ["ssim", "l2", "frames", "per_frame"] and s.pairs == 0
    assert res["ssim"] == 0.6 and res["l2"] == 3.0 and res["frames"] == 2
    s._pair_rows.append(torch.tensor([[1.0, 2.0, 3.0, 4.0, 0.5], [3.0, 4.0, 5.0, 6.0, 1.0]], dtype=torch.float64))
    res = s.result()
    assert list(res) == ["ssim", "l2", "frames", "per_frame", "warp_l1", "warp_mse", "truth_warp_l1", "truth_warp_mse",
                         "coverage", "pairs", "per_pair"]
    assert (res["warp_l1"], res["warp_mse"], res["truth_warp_l1"], res["truth_warp_mse"], res["coverage"]) == (2.0, 3.0, 4.0, 5.0, 0.75)
    assert res["pairs"] == s.pairs == 2 and res["per_pair"].shape == (2, 5)


def test_evaluate_scores_consecutive_outputs_along_the_flow_of_their_targets(monkeypatch):
    """``evaluate(temporal=stub)`` without a GPU: the translator's frame loop and the two kernels' entry points are
    replaced by their plain-torch restatements; what is checked is which frames meet which flow."""
    from ir2rgb_amd import metrics
    from ir2rgb_amd.inference import SequenceState, VideoTranslator, normalise_u8
    tG, H, W, n_in = 3, 8, 12, 7
    g = torch.Generator().manual_seed(5)
    targets = list(torch.randint(0, 256, (n_in, H, W, 3), generator=g, dtype=torch.uint8))
    outs = list(torch.randint(0, 256, (n_in - (tG - 1), H, W, 3), generator=g, dtype=torch.uint8))
    monkeypatch.setattr(metrics, "video_metrics", lambda o, p, r="reference": metrics.ssim_reference(o, p, r))
    monkeypatch.setattr(metrics, "warp_error", metrics.warp_error_reference)
    tr = VideoTranslator.__new__(VideoTranslator)
    tr.seq = SequenceState(tG)
    tr.translate = lambda frames, real_rgb=None: iter(outs)
    tr._rgb_frame = lambda frame, what: frame
    calls = []

    def stub(cur, prev):
        calls.append((cur, prev))
        k = len(calls)
        return make_flow(H, W, k).unsqueeze(0), make_weight("fractional", H, W, k).unsqueeze(0)

    plain = tr.evaluate(None, targets).result()
    assert not calls and list(plain) == ["ssim", "l2", "frames", "per_frame"]
    res = tr.evaluate(None, targets, temporal=stub).result()
    assert torch.equal(res["per_frame"], plain["per_frame"]) and res["ssim"] == plain["ssim"] and res["l2"] == plain["l2"]
    assert len(calls) == len(outs) - 1 == res["pairs"] and res["per_pair"].shape == (len(outs) - 1, 5)
    for k in range(1, len(outs)):
        cur, prev = calls[k - 1]
        t_cur, t_prev = targets[tG - 1 + k], targets[tG - 2 + k]
        assert cur.shape == (1, 3, H, W) and cur.dtype == torch.float32 and cur.is_contiguous()
        assert torch.equal(cur[0], normalise_u8(t_cur)) and torch.equal(prev[0], normalise_u8(t_prev))
        flow, conf = make_flow(H, W, k), make_weight("fractional", H, W, k)
        pred = metrics.warp_error_reference(outs[k - 1], outs[k], flow, conf)[0]
        truth = metrics.warp_error_reference(t_prev, t_cur, flow, conf)[0]
        assert torch.equal(res["per_pair"][k - 1], torch.stack([pred[0], pred[1], truth[0], truth[1], pred[2]]))
    means = res["per_pair"].mean(0).tolist()
    assert [res[k] for k in ("warp_l1", "warp_mse", "truth_warp_l1", "truth_warp_mse", "coverage")] == means
    with pytest.raises(TypeError, match="temporal"):
        tr.evaluate(None, targets, temporal=3)
