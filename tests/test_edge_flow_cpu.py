"""The FlowNet2 operator records (EDGE_FLOW of oracle/edge_records.py) checked without a GPU.

* The fp64 references of oracle/flow_ops_ref.py agree to 1e-12, at every record, with an independent fp64 formulation:
  oracle/closed_form.py in float64 and its autograd where the closed form applies (the FlowNetC cost volume; the warp and
  its flow gradient on planes of two or more rows and columns), a direct fp64 statement otherwise (general correlation
  parameters by F.pad and slices with autograd for the gradients; the warp, its flow gradient and the truncation-weight
  image gradient by loops over pixels, at every record, one-row, one-column and one-pixel planes included).  They also agree with the fp32
  C oracle (oracle/ops_ref.c) to its 1e-5 at the general-parameter and resample-backward records.
* corr_form restates the forward dispatch; every record's hand-written form equals it and every form has a record.
* Planted faults land over the bounds of oracle/replay_ops.py at a record of their kernel, and a float32 evaluation in
  another summation order stays under them (run with -s for the worst ratio per family).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from oracle import bounds as B
from oracle import closed_form as CF
from oracle import conv_ref as R
from oracle import edge_records as E
from oracle import flow_ops_ref as F
from oracle import ops as C_ORACLE
from oracle import replay_ops as G
from oracle.replay import gen, ids, np64, passes, rnd

RTOL = 1e-12
WORST = {}


def _recs(*entries, pred=lambda r: True):
    recs = [r for r in E.EDGE_FLOW if r["entry"] in entries and pred(r)]
    assert recs
    return pytest.mark.parametrize("rec", recs, ids=ids(recs))


def _close(got, want, what=""):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    scale = max(float(np.abs(want).max()), 1e-300) if want.size else 1.0
    err = float(np.abs(got - want).max()) if want.size else 0.0
    assert err <= RTOL * scale, f"{what}: differs by {err:.3g} (largest magnitude {scale:.3g})"


def _c_close(got, want, what):
    """The C oracle computes in fp32: its existing flat tolerance, 1e-5 of the largest magnitude (at least 1)."""
    err = float(np.abs(np.asarray(got, dtype=np.float64) - want).max())
    assert err <= 1e-5 * max(1.0, float(np.abs(want).max())), f"{what}: the C oracle differs by {err:.3g}"


def _note(family, ratio):
    WORST[family] = max(WORST.get(family, 0.0), ratio)


def _ratio(got, ref, bnd):
    ok, r, _, _ = B.check_bound(got, ref, bnd)
    return r


def _corr_args(rec):
    a = G.named_args(rec)
    if rec["entry"] == "ir2rgb_correlation_nhwc_half":
        return a, (20, 1, 20, 1, 2)
    return a, G.corr_geometry(a)


def _corr_inputs(rec, draw=False):
    a, geo = _corr_args(rec)
    g = gen(rec)
    shape = (a["N"], a["C"], a["H"], a["W"])
    mk = (lambda: R.draw(shape, g)) if draw else (lambda: torch.randn(shape, generator=g))
    return a, geo, mk().double(), mk().double(), g


def _corr_torch(f1, f2, pad, k, md, s1, s2):
    """Zero-pad both images, then for each displacement the k x k box sum (avg_pool2d) of the channel-summed product of
    f1 and the shifted f2, sampled at stride1."""
    N, Cc, H, W = f1.shape
    kr, d = (k - 1) // 2, md // s2
    _, oh, ow = F.correlation_out_shape(H, W, pad, k, md, s1, s2)
    big = md + kr + 1                                    # extra zeros so that every shifted slice exists
    p1, p2 = TF.pad(f1, (pad + big,) * 4), TF.pad(f2, (pad + big,) * 4)
    Hp, Wp = H + 2 * pad, W + 2 * pad
    outs = []
    for tj in range(-d, d + 1):
        for ti in range(-d, d + 1):
            lo, y2, x2 = big - kr, big - kr + tj * s2, big - kr + ti * s2      # a halo of kr: box q is centred at padded q
            prod = (p1[:, :, lo:lo + Hp + 2 * kr, lo:lo + Wp + 2 * kr]
                    * p2[:, :, y2:y2 + Hp + 2 * kr, x2:x2 + Wp + 2 * kr]).sum(1, keepdim=True)
            box = TF.avg_pool2d(prod, k, 1) * (k * k) if k > 1 else prod
            outs.append(box[:, :, md:md + (oh - 1) * s1 + 1:s1, md:md + (ow - 1) * s1 + 1:s1])
    return torch.cat(outs, 1) / (k * k * Cc)


def _independent_corr(f1, f2, geo):
    pad, k, md, s1, s2 = geo
    if k == 1 and s1 == 1 and pad == md:
        return CF.correlation(f1, f2, *geo)
    return _corr_torch(f1, f2, *geo)


# ---------------------------------------------------------------------------------------------------------------------
# references
@_recs("ir2rgb_correlation_fwd", "ir2rgb_correlation_nhwc_half")
def test_correlation_reference(rec):
    a, geo, f1, f2, _ = _corr_inputs(rec)
    ref, S = F.correlation(f1.numpy(), f2.numpy(), *geo)
    assert ref.shape[1:] == F.correlation_out_shape(a["H"], a["W"], *geo)
    _close(ref, _independent_corr(f1, f2, geo).numpy(), "correlation")
    _close(S, _independent_corr(f1.abs(), f2.abs(), geo).numpy(), "S")
    if rec["form"] == "generic:params":
        assert C_ORACLE.correlation_out_shape(a["C"], a["H"], a["W"], *geo) == ref.shape[1:]
        _c_close(C_ORACLE.correlation_fwd(f1.float().numpy(), f2.float().numpy(), *geo), F.correlation(
            np64(f1.float()), np64(f2.float()), *geo)[0], "correlation")


@_recs("ir2rgb_correlation_bwd")
def test_correlation_bwd_reference_is_the_adjoint(rec):
    a, geo, f1, f2, g = _corr_inputs(rec)
    pad, k, md, s1, s2 = geo
    f1, f2 = f1.float().double().requires_grad_(True), f2.float().double().requires_grad_(True)
    out = _independent_corr(f1, f2, geo)
    gout = torch.randn(out.shape, generator=g).double()
    out.backward(gout)
    g1, g2, S1, S2, L1, L2 = F.correlation_bwd(f1.detach().numpy(), f2.detach().numpy(), gout.numpy(), pad, k, md, s2)
    _close(g1, f1.grad.numpy(), "gin1")
    _close(g2, f2.grad.numpy(), "gin2")
    assert (S1 >= np.abs(g1) * (1 - 1e-12)).all() and (S2 >= np.abs(g2) * (1 - 1e-12)).all()
    assert L1.max() <= out.shape[1] * k * k and L2.max() <= out.shape[1] * k * k and L1.max() > 0
    if rec["form"] != "bwd:fast":
        c1, c2 = C_ORACLE.correlation_bwd(f1.detach().numpy(), f2.detach().numpy(), gout.numpy(), *geo)
        _c_close(c1, g1, "gin1")
        _c_close(c2, g2, "gin2")


def _resample_inputs(rec):
    g = gen(rec)
    a, img, flow = G._resample_inputs(rec, g)
    return a, img.double(), flow.double(), torch.randn(img.shape, generator=g).double()


def _gimg_loop(img, flow, gout, dtype=np.float64, reverse=False):
    """The image gradient pixel by pixel: coordinates as fp32 sums, truncation weights, contributions added in pixel order
    (or the reverse) in ``dtype``."""
    N, Cc, H, W = img.shape
    out = np.zeros((N, Cc, H, W), dtype=dtype)
    pix = [(n, y, x) for n in range(N) for y in range(H) for x in range(W)]
    for n, y, x in (pix[::-1] if reverse else pix):
        xf, yf = np.float32(x) + np.float32(flow[n, 0, y, x]), np.float32(y) + np.float32(flow[n, 1, y, x])
        fx, fy = int(np.floor(xf)), int(np.floor(yf))
        xL, xR, yT, yB = min(max(fx, 0), W - 1), min(max(fx + 1, 0), W - 1), min(max(fy, 0), H - 1), min(max(fy + 1, 0), H - 1)
        a, b = dtype(xf - np.float32(int(xf))), dtype(yf - np.float32(int(yf)))
        go = gout[n, :, y, x].astype(dtype)
        one = dtype(1)
        out[n, :, yT, xL] += (one - a) * (one - b) * go
        out[n, :, yT, xR] += a * (one - b) * go
        out[n, :, yB, xL] += (one - a) * b * go
        out[n, :, yB, xR] += a * b * go
    return out


def _warp_loop(img, flow, gout):
    """The forward and the flow gradient pixel by pixel in fp64 on exact coordinates: floor weights, corner indices
    clamped.  -> (warped, gflow)."""
    N, Cc, H, W = img.shape
    v, gf = np.zeros((N, Cc, H, W)), np.zeros((N, 2, H, W))
    for n in range(N):
        for y in range(H):
            for x in range(W):
                xf, yf = x + float(flow[n, 0, y, x]), y + float(flow[n, 1, y, x])
                fx, fy = int(np.floor(xf)), int(np.floor(yf))
                al, be = xf - fx, yf - fy
                xL, xR = min(max(fx, 0), W - 1), min(max(fx + 1, 0), W - 1)
                yT, yB = min(max(fy, 0), H - 1), min(max(fy + 1, 0), H - 1)
                for c in range(Cc):
                    tl, tr, bl, br = img[n, c, yT, xL], img[n, c, yT, xR], img[n, c, yB, xL], img[n, c, yB, xR]
                    v[n, c, y, x] = (1 - al) * (1 - be) * tl + al * (1 - be) * tr + (1 - al) * be * bl + al * be * br
                    go = gout[n, c, y, x]
                    gf[n, 0, y, x] += go * ((1 - be) * (tr - tl) + be * (br - bl))
                    gf[n, 1, y, x] += go * ((1 - al) * (bl - tl) + al * (br - tr))
    return v, gf


@_recs("ir2rgb_resample2d_fwd", "ir2rgb_resample2d_bwd")
def test_resample_references(rec):
    a, img, flow, gout = _resample_inputs(rec)
    v, _, _, S = F.resample2d(img.numpy(), flow.numpy())
    fl = flow.clone().requires_grad_(True)
    im = img.clone().requires_grad_(True)
    want = CF.resample2d(im, fl)
    lv, lgf = _warp_loop(img.numpy(), flow.numpy(), gout.numpy())
    _close(v, lv, "warped (loop)")
    if a["W"] > 1 and a["H"] > 1:          # (grid_sample's normalisation needs two samples per axis: the closed form too)
        _close(v, want.detach().numpy(), "warped")
    if rec["entry"] == "ir2rgb_resample2d_fwd":
        return
    r = F.resample2d_bwd(img.numpy(), flow.numpy(), gout.numpy())
    _close(r["gimg"], _gimg_loop(img.numpy(), flow.numpy(), gout.numpy()), "gimg")
    assert r["L"].sum() == 4 * a["N"] * a["H"] * a["W"]
    _close(r["gflow"], lgf, "gflow (loop)")
    if a["W"] > 1 and a["H"] > 1:
        want.backward(gout)
        _close(r["gflow"], fl.grad.numpy(), "gflow")
    ci, cf = C_ORACLE.resample2d_bwd(img.numpy(), flow.numpy(), gout.numpy())
    _c_close(ci, r["gimg"], "gimg")
    _c_close(cf, r["gflow"], "gflow")
    if "far" in rec:                       # one border column / row takes every contribution
        assert r["L"].max() >= 2 * (a["W"] if rec["far"][0] else a["H"])
        assert not r["gflow"][:, 0 if rec["far"][0] else 1].any()


@_recs("ir2rgb_channelnorm_bwd")
def test_channelnorm_bwd_reference(rec):
    a, x, out, gout = G.channelnorm_bwd_inputs(rec, gen(rec))
    ref, _ = F.channelnorm_bwd(np64(x), np64(out), np64(gout))
    want = torch.stack([gout[:, 0].double() * x[:, c].double() / (out[:, 0].double() + 1e-9) for c in range(a["C"])], 1)
    _close(ref, want.numpy(), "channelnorm_bwd")
    _close(np64(out), CF.channelnorm(x.double()).float().numpy(), "out")
    assert not ref[0, :, 0, 0].any()
    _c_close(C_ORACLE.channelnorm_bwd(x.numpy(), out.numpy(), gout.numpy()), ref, "channelnorm_bwd")
    if "scale" in rec:                     # the 1e-9 matters: without it the gradient is ~10 % larger
        xa = torch.autograd.Variable(x.double(), requires_grad=True)
        CF.channelnorm(xa).backward(gout.double())
        rel = np.abs(xa.grad.numpy() - ref)[1] / np.abs(ref)[1]
        assert 0.01 < np.median(rel) < 0.5


# ---------------------------------------------------------------------------------------------------------------------
# forms
def test_every_flow_form_has_a_record_and_the_dispatch_is_restated():
    assert {r["form"] for r in E.EDGE_FLOW} == set(E.FLOW_FORMS)
    for r in E.EDGE_FLOW:
        if r["entry"] == "ir2rgb_correlation_fwd":
            a = G.named_args(r)
            want = E.corr_form(a["N"], a["C"], a["H"], a["W"], *G.corr_geometry(a), aligned=not r.get("offset"))
            assert r["form"] == want, (r, want)
    assert {r["entry"] for r in E.EDGE_FLOW} == {
        "ir2rgb_correlation_fwd", "ir2rgb_correlation_bwd", "ir2rgb_correlation_nhwc_half", "ir2rgb_resample2d_fwd",
        "ir2rgb_resample2d_bwd", "ir2rgb_channelnorm_bwd"}
    assert all(r in E.EDGE for r in E.EDGE_FLOW)


def test_mfma_records_are_what_the_entry_accepts():
    """The argument checks of ir2rgb_correlation_nhwc_half (correlation_mfma.hip:192-199)."""
    for r in E.EDGE_FLOW:
        if r["entry"] != "ir2rgb_correlation_nhwc_half":
            continue
        a = G.named_args(r)
        assert a["C"] in (128, 256) and 1 <= a["W"] <= 128 and r["modes"] == [0, 1]
        assert not (a["lda"] | a["offa"] | a["ldb"] | a["offb"]) & 7
        assert a["offa"] + a["C"] <= a["lda"] and a["offb"] + a["C"] <= a["ldb"] and 0 <= a["offo"] <= a["ldo"] - 441


# ---------------------------------------------------------------------------------------------------------------------
# faults: each must land over the bound at one record of its kernel at least, the unfaulted rounding under it everywhere
def _fwd_case(rec):
    a, geo, f1, f2, _ = _corr_inputs(rec)
    f1, f2 = np64(f1.float()), np64(f2.float())
    ref, S = F.correlation(f1, f2, *geo)
    return a, geo, f1, f2, ref, B.bound_sum(ref, S, "f32", geo[1] ** 2 * a["C"] + 2)


def _drop_channel(a, geo, f1, f2, ref):
    g1 = f1.copy()
    g1[:, a["C"] // 2] = 0
    return F.correlation(g1, f2, *geo)[0]


def _drop_group(a, geo, f1, f2, ref):
    if a["C"] < 16:
        return None
    g1 = f1.copy()
    g1[:, -8:] = 0
    return F.correlation(g1, f2, *geo)[0]


def _disp(ref):
    D = int(round(ref.shape[1] ** 0.5))
    return ref.reshape(ref.shape[0], D, D, *ref.shape[2:])


def _xchunks_swapped(a, geo, f1, f2, ref):
    if a["W"] <= 128:
        return None
    bad = ref.copy()
    n = a["W"] - 128
    bad[..., 128:], bad[..., :n] = ref[..., :n], ref[..., 128:]
    return bad


CORR_FAULTS = {
    "one channel dropped": _drop_channel,
    "the last 8-channel group dropped": _drop_group,
    "the border clamped instead of zero": lambda a, geo, f1, f2, ref: F.correlation(f1, f2, *geo, clamp_border=True)[0],
    "ti off by one": lambda a, geo, f1, f2, ref: np.roll(_disp(ref), 1, 2).reshape(ref.shape),
    "tj and ti swapped": lambda a, geo, f1, f2, ref: _disp(ref).transpose(0, 2, 1, 3, 4).reshape(ref.shape),
    "two x chunks swapped": _xchunks_swapped,
    "scale 1 / C instead of 1 / (k^2 C)": lambda a, geo, f1, f2, ref: ref * geo[1] ** 2 if geo[1] > 1 else None,
}


@pytest.mark.parametrize("fault", list(CORR_FAULTS))
def test_correlation_fault_rejected(fault):
    kernels = {}
    for rec in [r for r in E.EDGE_FLOW if r["entry"] == "ir2rgb_correlation_fwd"]:
        a, geo, f1, f2, ref, bnd = _fwd_case(rec)
        assert passes(rnd(ref, "f32"), ref, bnd)
        bad = CORR_FAULTS[fault](a, geo, f1, f2, ref)
        if bad is not None:
            k = rec["form"].split(":")[0]
            kernels[k] = kernels.get(k, False) or not passes(rnd(bad, "f32"), ref, bnd)
    assert kernels and all(kernels.values()), (fault, kernels)


def _mfma_case(rec):
    a, geo, f1, f2, g = _corr_inputs(rec, draw=True)
    ref, S = F.correlation(f1.numpy(), f2.numpy(), *geo)
    return a, f1.numpy(), f2.numpy(), ref, S, g


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("fault", ["parity swapped", "slope not applied", "offb ignored"])
def test_mfma_fault_rejected(fault, fmt):
    caught = 0
    for rec in [r for r in E.EDGE_FLOW if r["entry"] == "ir2rgb_correlation_nhwc_half"]:
        a, f1, f2, ref, S, g = _mfma_case(rec)
        want = G.leaky(ref, a["slope"])
        for ofmt, w in (("f32", ref), (fmt, want)):
            assert passes(rnd(w, ofmt), w, B.bound(w, S, ofmt, a["C"] + 2))
        bnd0, bnd1 = B.bound(ref, S, "f32", a["C"] + 2), B.bound(want, S, fmt, a["C"] + 2)
        if fault == "parity swapped" and a["W"] % 2 == 0:
            swap = ref.reshape(*ref.shape[:3], -1, 2)[..., ::-1].reshape(ref.shape)
            assert not passes(rnd(swap, "f32"), ref, bnd0) and not passes(rnd(G.leaky(swap, a["slope"]), fmt), want, bnd1)
            caught += 1
        if fault == "slope not applied" and a["slope"] != 1.0:      # (a one-column record may hold no negative value)
            caught += not passes(rnd(ref, fmt), want, bnd1)
        if fault == "offb ignored" and a["offb"]:
            buf = R.draw((a["N"], a["ldb"], a["H"], a["W"]), g).double().numpy()
            buf[:, a["offb"]:a["offb"] + a["C"]] = f2
            bad = F.correlation(f1, buf[:, :a["C"]], 20, 1, 20, 1, 2)[0]
            assert not passes(rnd(bad, "f32"), ref, bnd0) and not passes(rnd(G.leaky(bad, a["slope"]), fmt), want, bnd1)
            caught += 1
    assert caught


@_recs("ir2rgb_resample2d_bwd")
def test_truncation_weights_cannot_be_told_from_floor_weights(rec):
    """The image gradient's weights use xf - trunc(xf), which differs from the floor fraction below zero only -- where both
    corners of that axis clamp onto the border pixel and receive (1 - a) + a = 1 of the value whatever a is.  A kernel with
    floor weights therefore computes the same image gradient: that fault is not observable, at any record, by any bound
    (its rounding differs, inside the bound)."""
    a, img, flow, gout = _resample_inputs(rec)
    args = (img.numpy(), flow.numpy(), gout.numpy())
    r, bad = F.resample2d_bwd(*args), F.resample2d_bwd(*args, fault="floor")
    assert np.abs(bad["gimg"] - r["gimg"]).max() <= 1e-12 * max(1.0, r["S_gimg"].max())
    if "far" in rec and rec["far"][1] < 0:
        xf, yf = F.pixel_coords(flow.numpy())
        assert (yf < 0).all() and np.abs((yf - np.trunc(yf)) - (yf - np.floor(yf))).min() == 1.0


@pytest.mark.parametrize("fault", ["corner", "lose"])
def test_resample_bwd_fault_rejected(fault):
    caught = 0
    for rec in [r for r in E.EDGE_FLOW if r["entry"] == "ir2rgb_resample2d_bwd"]:
        a, img, flow, gout = _resample_inputs(rec)
        args = (img.numpy(), flow.numpy(), gout.numpy())
        r = F.resample2d_bwd(*args)
        bi, bf = G.resample_bwd_bounds(r, a["C"], a["H"], a["W"])
        assert passes(rnd(r["gimg"], "f32"), r["gimg"], bi) and passes(rnd(r["gflow"], "f32"), r["gflow"], bf)
        if fault == "lose":
            if "far" not in rec:
                continue
            bad = F.resample2d_bwd(*args, fault=("lose", a["H"] * a["W"] // 2 + 3))["gimg"]
            assert not passes(rnd(bad, "f32"), r["gimg"], bi), rec
            caught += 1
        else:
            bad = F.resample2d_bwd(*args, fault=fault)["gimg"]
            caught += not passes(rnd(bad, "f32"), r["gimg"], bi)
    assert caught >= 2, caught


def test_channelnorm_bwd_without_the_1e_9_rejected():
    rec = next(r for r in E.EDGE_FLOW if r.get("scale"))
    a, x, out, gout = G.channelnorm_bwd_inputs(rec, gen(rec))
    ref, _ = F.channelnorm_bwd(np64(x), np64(out), np64(gout))
    bnd = 3 * B.U32 * np.abs(ref) + B.ETA["f32"]
    assert passes(rnd(ref, "f32"), ref, bnd)
    with np.errstate(divide="ignore", invalid="ignore"):
        bad = np.nan_to_num(np64(gout) * np64(x) / np64(out))
    assert not passes(rnd(bad, "f32"), ref, bnd)


# ---------------------------------------------------------------------------------------------------------------------
# float32 evaluations in another order stay under the bounds
@_recs("ir2rgb_correlation_fwd", "ir2rgb_correlation_nhwc_half")
def test_correlation_float32_in_reversed_channel_order_is_inside(rec):
    mfma = rec["entry"] == "ir2rgb_correlation_nhwc_half"
    a, geo, f1, f2, _ = _corr_inputs(rec, draw=mfma)
    f1, f2 = f1.float(), f2.float()
    ref, S = F.correlation(np64(f1), np64(f2), *geo)
    got = np64(torch.from_numpy(F.correlation(f1.numpy()[:, ::-1].copy(), f2.numpy()[:, ::-1].copy(), *geo)[0]))
    if not mfma:
        _note(rec["form"].split(":")[0], _ratio(got, ref, B.bound_sum(ref, S, "f32", geo[1] ** 2 * a["C"] + 2)))
        assert passes(got, ref, B.bound_sum(ref, S, "f32", geo[1] ** 2 * a["C"] + 2))
        return
    want = G.leaky(ref, a["slope"])
    for fmt in ("bf16", "f16"):
        g1 = rnd(np64(torch.from_numpy(G.leaky(got, a["slope"]).astype(np.float32))), fmt)
        _note("mfma", max(_ratio(got, ref, B.bound(ref, S, "f32", a["C"] + 2)), _ratio(g1, want, B.bound(want, S, fmt, a["C"] + 2))))
        assert passes(got, ref, B.bound(ref, S, "f32", a["C"] + 2)) and passes(g1, want, B.bound(want, S, fmt, a["C"] + 2))


@_recs("ir2rgb_correlation_bwd")
def test_correlation_bwd_float32_in_reversed_order_is_inside(rec):
    """corr_bwd_kernel's own arithmetic (a float32 window sum times the other image's pixel, accumulated over tc) with tc
    descending."""
    a, geo, f1, f2, g = _corr_inputs(rec)
    pad, k, md, s1, s2 = geo
    kr, d = (k - 1) // 2, md // s2
    D = 2 * d + 1
    N, Cc, H, W = f1.shape
    oc, oh, ow = F.correlation_out_shape(H, W, *geo)
    f1, f2 = f1.float().numpy(), f2.float().numpy()
    gout = torch.randn(N, oc, oh, ow, generator=g).numpy()
    r1, r2, S1, S2, L1, L2 = F.correlation_bwd(f1.astype(np.float64), f2.astype(np.float64), gout.astype(np.float64), pad, k, md, s2)
    g1, g2 = np.zeros_like(f1), np.zeros_like(f2)
    for by in range(H):
        for bx in range(W):
            for tc in reversed(range(oc)):
                j2, i2 = (tc // D - d) * s2, (tc % D - d) * s2
                for sign, f, out in ((1, f2, g1), (-1, f1, g2)):
                    yy, xx = by + sign * j2, bx + sign * i2
                    lo_y, lo_x = by + pad - kr - md - (j2 if sign < 0 else 0), bx + pad - kr - md - (i2 if sign < 0 else 0)
                    ys, xs = slice(max(lo_y, 0), max(min(lo_y + 2 * kr + 1, oh), 0)), slice(max(lo_x, 0), max(min(lo_x + 2 * kr + 1, ow), 0))
                    if 0 <= yy < H and 0 <= xx < W:
                        win = gout[:, tc, ys, xs][:, ::-1, ::-1].reshape(N, -1)
                        s = np.zeros(N, dtype=np.float32)
                        for e in range(win.shape[1]):
                            s += win[:, e]
                        out[:, :, by, bx] += s[:, None] * f[:, :, yy, xx]
    inv = np.float32(1.0) / np.float32(k * k * Cc)
    for got, ref, S, L in ((g1 * inv, r1, S1, L1), (g2 * inv, r2, S2, L2)):
        bnd = B.bound_sum(ref, S, "f32", L + 2)
        _note("bwd", _ratio(got.astype(np.float64), ref, bnd))
        assert passes(got.astype(np.float64), ref, bnd)


@_recs("ir2rgb_resample2d_bwd")
def test_resample_bwd_float32_in_reversed_order_is_inside(rec):
    a, img, flow, gout = _resample_inputs(rec)
    r = F.resample2d_bwd(img.numpy(), flow.numpy(), gout.numpy())
    bi, bf = G.resample_bwd_bounds(r, a["C"], a["H"], a["W"])
    gimg = _gimg_loop(img.numpy(), flow.numpy(), gout.numpy(), dtype=np.float32, reverse=True).astype(np.float64)
    _note("gimg", _ratio(gimg, r["gimg"], bi))
    assert passes(gimg, r["gimg"], bi)
    # the flow gradient in float32 on float32 coordinates, channels reversed
    N, Cc, H, W = img.shape
    im, go, fl = (t.float().numpy() for t in (img, gout, flow))
    xf, yf = F.pixel_coords(fl)
    xf, yf = xf.astype(np.float32), yf.astype(np.float32)
    fx, fy = np.floor(xf), np.floor(yf)
    al, be = xf - fx, yf - fy
    xL, xR = np.clip(fx, 0, W - 1).astype(int), np.clip(fx + 1, 0, W - 1).astype(int)
    yT, yB = np.clip(fy, 0, H - 1).astype(int), np.clip(fy + 1, 0, H - 1).astype(int)
    n = np.arange(N)[:, None, None]
    ox, oy = np.zeros((N, H, W), np.float32), np.zeros((N, H, W), np.float32)
    one = np.float32(1)
    for c in reversed(range(Cc)):
        pl, gc = im[:, c], go[:, c]
        tl, tr, bl, br = pl[n, yT, xL], pl[n, yT, xR], pl[n, yB, xL], pl[n, yB, xR]
        ox += be * gc * br; ox -= be * gc * bl; ox += (one - be) * gc * tr; ox -= (one - be) * gc * tl
        oy += al * gc * br; oy -= al * gc * tr; oy += (one - al) * gc * bl; oy -= (one - al) * gc * tl
    got = np.stack([ox, oy], 1).astype(np.float64)
    _note("gflow", _ratio(got, r["gflow"], bf))
    assert passes(got, r["gflow"], bf)


@_recs("ir2rgb_resample2d_fwd")
def test_resample_fwd_float32_is_inside(rec):
    a, img, flow, _ = _resample_inputs(rec)
    N, Cc, H, W = img.shape
    v, dvx, dvy, S = F.resample2d(img.numpy(), flow.numpy())
    bnd = B.C_AR * B.U32 * S + dvx * B.coord_delta(W) + dvy * B.coord_delta(H) + B.ETA["f32"]
    xf, yf = (t.astype(np.float32) for t in F.pixel_coords(flow.numpy()))
    fx, fy = np.floor(xf), np.floor(yf)
    al, be = xf - fx, yf - fy
    xL, xR = np.clip(fx, 0, W - 1).astype(int), np.clip(fx + 1, 0, W - 1).astype(int)
    yT, yB = np.clip(fy, 0, H - 1).astype(int), np.clip(fy + 1, 0, H - 1).astype(int)
    n = np.arange(N)[:, None, None]
    one = np.float32(1)
    im = img.float().numpy()
    got = np.stack([al * be * im[:, c][n, yB, xR] + (one - al) * be * im[:, c][n, yB, xL] + al * (one - be) * im[:, c][n, yT, xR]
                    + (one - al) * (one - be) * im[:, c][n, yT, xL] for c in range(Cc)], 1).astype(np.float64)
    _note("resample_fwd", _ratio(got, v, bnd))
    assert passes(got, v, bnd)


@_recs("ir2rgb_channelnorm_bwd")
def test_channelnorm_bwd_float32_is_inside(rec):
    a, x, out, gout = G.channelnorm_bwd_inputs(rec, gen(rec))
    ref, _ = F.channelnorm_bwd(np64(x), np64(out), np64(gout))
    got = ((gout.numpy() * x.numpy()).astype(np.float64) / (out.numpy().astype(np.float64) + 1e-9)).astype(np.float32)
    bnd = 3 * B.U32 * np.abs(ref) + B.ETA["f32"]
    _note("channelnorm_bwd", _ratio(got.astype(np.float64), ref, bnd))
    assert passes(got.astype(np.float64), ref, bnd)


def teardown_module(module):
    if WORST:
        print("\nfloat32 re-evaluations, worst err/bound per family: " + ", ".join(f"{k} {v:.4f}" for k, v in sorted(WORST.items())))
