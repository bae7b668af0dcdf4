"""The comparators of oracle/replay_ops.py must catch the bugs they are there for, and every entry point the window
launches must be checked somewhere (no GPU).

At geometries of tests/window_geometries.json, fp64 "faulty outputs" are built from oracle/window_ops_ref.py -- a
dropped reflection mirror, a wrong activation nibble, the align_corners lattice "fixed", a clamped pixel that keeps its
flow gradient, count_include_pad pooling, a loss mean over a rounded n, Adam without bias correction or with an
un-updated n % 4 tail, swapped up-sampler taps -- and the bounds of oracle/bounds.py must reject each one, while the
unfaulted reference rounded to the output format passes.
"""
import numpy as np
import pytest
import torch

from oracle import bounds as B
from oracle import replay_ops as G
from oracle import window as WG
from oracle import window_ops_ref as O
from oracle.replay import passes, rnd

OPS = WG.op_entries()


def _pick(entry, pred=lambda a: True):
    for r in OPS:
        if r["entry"] == entry and ("args" not in r or pred(G.named_args(r))) and ("args" in r or pred(r)):
            return r
    raise LookupError(entry)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------------------------------
# completeness
def test_every_entry_point_is_classified():
    from ir2rgb_amd import _lib
    classes = {n: WG.entry_class(n) for n in _lib.PROTOTYPES}
    assert set(classes.values()) <= {"conv", "bn", "pack", "query", "op"}
    assert {n for n, c in classes.items() if c == "conv"} == set(WG.CONV_ENTRIES)
    assert {n for n, c in classes.items() if c == "bn"} == set(WG.BN_ENTRIES)
    assert {n for n, c in classes.items() if c == "pack"} == set(WG.PACK_ENTRIES)
    for n, c in classes.items():        # a query returns a size / name; everything that launches is recorded or packs
        if c == "query":
            assert _lib.PROTOTYPES[n][0] is not _lib.c_int or not any(t is _lib.c_void_p for t in _lib.PROTOTYPES[n][1]), n


def test_every_op_record_is_replayed_or_covered():
    """Every op entry of the window has a replay (none is covered elsewhere any more)."""
    entries = {r["entry"] for r in OPS}
    assert entries, "the manifest holds no op records"
    missing = sorted(e for e in entries if e not in G.REPLAY)
    assert not missing, "op entries not in oracle/replay_ops.py's REPLAY: " + ", ".join(missing)
    for e in entries:
        if "args" in next(r for r in OPS if r["entry"] == e):
            assert e in G.ARGS, e


def test_argument_names_match_the_prototypes():
    """named_args and edge_records.op zip ARGS with a record's arguments or the prototype's types, and zip stops at the
    shorter: a name too few or too many would shift or drop an argument silently."""
    from ir2rgb_amd import _lib
    for entry, names in G.ARGS.items():
        assert len(names.split()) == len(_lib.PROTOTYPES[entry][1]) - 1, entry      # (the stream has no name)


def test_launch_ids_of_op_records():
    ids = [WG.launch_id(r) for r in OPS]
    assert all(i and " " not in i for i in ids)


# ---------------------------------------------------------------------------------------------------------------------
# head_finish / head_finish_bwd
@pytest.fixture(scope="module")
def head():
    rec = _pick("ir2rgb_head_finish", lambda a: any(O.nibble(a["acts"], c) == 0 for c in range(a["Cout"])))
    a = G.named_args(rec)
    a = dict(a, N=1)
    g = _gen(3)
    T = torch.randn(1, a["H"], a["W"], a["CT"], generator=g, dtype=torch.float64).numpy() * 0.5
    bias = torch.randn(a["Cout"], generator=g, dtype=torch.float64).numpy() * 0.5
    out, pre, S = O.head_finish(T, bias, a["Cout"], a["KH"], a["pad_h"], a["acts"], a["mul"])
    bnd = B.bound_act(out, O.act_slope(out, a["acts"], a["mul"], a["Cout"]), S, a["KH"] + 1)
    return a, T, bias, out, pre, bnd


def test_head_finish_unfaulted_passes(head):
    a, T, bias, out, pre, bnd = head
    assert passes(rnd(out, "f32"), out, bnd)


def test_head_finish_sigmoid_on_flow_channel_rejected(head):
    a, T, bias, out, pre, bnd = head
    co = next(c for c in range(a["Cout"]) if O.nibble(a["acts"], c) == 0)
    bad = out.copy()
    bad[:, co] = 1 / (1 + np.exp(-pre[:, co]))
    assert not passes(rnd(bad, "f32"), out, bnd)


def test_head_finish_dropped_tile_edge_rejected(head):
    """The last 8-row / 16-column tile of the image left out (the image's right- and bottom-most outputs unwritten)."""
    a, T, bias, out, pre, bnd = head
    bad = out.copy()
    bad[..., a["H"] - 1 - (a["H"] - 1) % 8:, :] = 0
    bad[..., a["W"] - 1 - (a["W"] - 1) % 16:] = 0
    assert not passes(rnd(bad, "f32"), out, bnd)


@pytest.fixture(scope="module")
def head_bwd():
    rec = _pick("ir2rgb_head_finish_bwd")
    a = dict(G.named_args(rec), N=1)
    g = _gen(4)
    shape = (1, a["Cout"], a["H"], a["W"])
    pre = torch.randn(shape, generator=g, dtype=torch.float64).numpy() * 2
    out = np.empty(shape)
    for co in range(a["Cout"]):
        nb = O.nibble(a["acts"], co)
        out[:, co] = np.tanh(pre[:, co]) if nb == 1 else (1 / (1 + np.exp(-pre[:, co])) if nb == 2 else pre[:, co] * a["mul"])
    out = rnd(out, "f32")
    gout = rnd(torch.randn(shape, generator=g, dtype=torch.float64).numpy(), "f32")
    dT, db, S, Sb = O.head_finish_bwd(gout, out, a["Cout"], a["KH"], a["CT"], a["pad_h"], a["acts"], a["mul"])
    return a, gout, out, dT, S


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_head_finish_bwd_unfaulted_passes(head_bwd, fmt):
    a, gout, out, dT, S = head_bwd
    assert passes(rnd(dT, fmt), dT, B.bound_rw(dT, S, fmt, 3, 6))


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("edge", ["top", "bottom"])
def test_head_finish_bwd_missing_mirror_rejected(head_bwd, fmt, edge):
    """Output row 0 (H-1) reads rows 1..pad (H-2..H-1-pad) through the mirror: drop one of those contributions."""
    a, gout, out, dT, S = head_bwd
    H, pad, KH = a["H"], a["pad_h"], a["KH"]
    bad = dT.copy()
    y = 0 if edge == "top" else H - 1
    ky = 0 if edge == "top" else KH - 1            # t = y + ky - pad lies beyond the edge
    t = y + ky - pad
    dst = int(O.refl(np.array([t]), H)[0])
    assert dst != y
    o, g = out[:, 0, y], gout[:, 0, y]
    nb = O.nibble(a["acts"], 0)
    d = g * (1 - o * o) if nb == 1 else (g * o * (1 - o) if nb == 2 else g * a["mul"])
    bad[:, dst, :, ky] -= d
    assert not passes(rnd(bad, fmt), dT, B.bound_rw(dT, S, fmt, 3, 6))


# ---------------------------------------------------------------------------------------------------------------------
# warp_blend
@pytest.fixture(scope="module")
def warp():
    rec = _pick("ir2rgb_warp_blend_bwd")
    a = G.named_args(rec)
    N, Cp, H, W = 1, a["Cp"], a["H"], a["W"]
    raw, prev, flow, w = (t.double().numpy() for t in G._warp_inputs(N, Cp, H, W, _gen(5)))
    gout = torch.randn(N, 3, H, W, generator=_gen(6), dtype=torch.float64).numpy()
    r = O.warp_blend(raw, prev, flow, w, gout=gout)
    dx, dy = B.coord_delta(W), B.coord_delta(H)
    bout = B.C_AR * B.U32 * r["S_out"] + r["dout_dix"] * dx + r["dout_diy"] * dy + B.ETA["f32"]
    bgf = B.C_AR * B.U32 * r["S_gflow"] + np.stack([r["dgflow_x_diy"] * dy, r["dgflow_y_dix"] * dx], 1) + B.ETA["f32"]
    return (raw, prev, flow, w, gout), r, bout, bgf


def test_warp_blend_unfaulted_passes(warp):
    _, r, bout, bgf = warp
    assert passes(rnd(r["out"], "f32"), r["out"], bout)
    assert passes(rnd(r["gflow"], "f32"), r["gflow"], bgf)


def test_warp_blend_align_corners_lattice_rejected(warp):
    (raw, prev, flow, w, gout), r, bout, _ = warp
    bad = O.warp_blend(raw, prev, flow, w, align_corners_true=True)["out"]
    assert not passes(rnd(bad, "f32"), r["out"], bout)


def test_warp_blend_clamped_flow_gradient_rejected(warp):
    (raw, prev, flow, w, gout), r, _, bgf = warp
    bad = O.warp_blend(raw, prev, flow, w, gout=gout, keep_clamped_grad=True)["gflow"]
    clamped = ~((r["ix"] > 0) & (r["ix"] < w.shape[3] - 1))
    assert clamped.any()
    assert not passes(rnd(bad, "f32"), r["gflow"], bgf)


# ---------------------------------------------------------------------------------------------------------------------
# avgpool3s2
@pytest.mark.parametrize("backward", [0, 1])
def test_avgpool_count_include_pad_rejected(backward):
    rec = _pick("ir2rgb_avgpool3s2", lambda a: a["backward"] == backward)
    a = G.named_args(rec)
    P, H, W = min(a["planes"], 2), a["H"], a["W"]
    g = _gen(7)
    if not backward:
        x = torch.randn(P, H, W, generator=g, dtype=torch.float64).numpy()
        ref, S = O.avgpool3s2(x)
        bad, _ = O.avgpool3s2(x, count_include_pad=True)
        bnd = B.bound_sum(ref, S, "f32", 10)
    else:
        gy = torch.randn(P, (H - 1) // 2 + 1, (W - 1) // 2 + 1, generator=g, dtype=torch.float64).numpy()
        ref, S = O.avgpool3s2_bwd(gy, H, W)
        bad, _ = O.avgpool3s2_bwd(gy, H, W, count_include_pad=True)
        bnd = B.bound_sum(ref, S, "f32", 8)
    assert set(np.unique(O.avgpool_divisors(H)[:, None] * O.avgpool_divisors(W)[None, :])) <= {1, 2, 3, 4, 6, 9}
    assert passes(rnd(ref, "f32"), ref, bnd)
    assert not passes(rnd(bad, "f32"), ref, bnd)


# ---------------------------------------------------------------------------------------------------------------------
# grouped losses
def test_loss_mean_over_rounded_n_rejected():
    """A term whose mean divides by n rounded up to its blocks' slice multiple, at every recorded term."""
    caught = 0
    for rec in [r for r in OPS if r["entry"] == "ir2rgb_loss_multi_fwd"]:
        for i, it in enumerate(rec["items"]):
            n = it["n"]
            chain = G.loss_chain(rec, i)
            ns = [t["n"] for t in rec["items"]]
            nb = min(int((G.LOSS_BLOCKS - len(ns)) * n / float(sum(ns))) + 1, -(-n // 2048))
            unit = 8 * nb if it["kind"] == 0 else nb
            n_bad = -(-n // unit) * unit if n % unit else n + unit
            ref = 1.0               # an all-positive mean: S = |ref|
            bad = ref * n / n_bad
            bnd = B.bound_rw(np.array([ref]), np.array([ref]), "f32", chain, 4)
            assert passes(np.float32(ref), np.array([ref]), bnd)
            assert not passes(np.array([np.float32(bad)], dtype=np.float64), np.array([ref]), bnd), (n, n_bad, chain)
            caught += 1
    assert caught


# ---------------------------------------------------------------------------------------------------------------------
# Adam
@pytest.fixture(scope="module")
def adam_rec():
    return _pick("ir2rgb_adam_step")


def _adam_case(rec, n, step, **kw):
    g = _gen(8)
    p = rnd(torch.randn(n, generator=g, dtype=torch.float64).numpy() * 0.05, "f32")
    gr = rnd(torch.randn(n, generator=g, dtype=torch.float64).numpy() * 0.01, "f32")
    m = np.zeros(n) if step == 1 else rnd(torch.randn(n, generator=g, dtype=torch.float64).numpy() * 0.01, "f32")
    v = np.zeros(n) if step == 1 else rnd(torch.rand(n, generator=g, dtype=torch.float64).numpy() * 1e-4, "f32")
    b1, b2 = float(np.float32(rec["beta1"])), float(np.float32(rec["beta2"]))
    args = (p, gr, m, v, rec["lr"], b1, b2, rec["eps"], step)
    p1, m1, v1, upd, Sm, ss, den = O.adam(*args)
    bm = 4 * B.U32 * Sm + B.ETA["f32"]
    bp = B.U32 * np.abs(p1) + 16 * B.U32 * upd + ss * bm / den + B.ETA["f32"]
    return args, p1, bp


@pytest.mark.parametrize("step", [1, 14])
def test_adam_without_bias_correction_rejected(adam_rec, step):
    args, p1, bp = _adam_case(adam_rec, 4099, step)
    assert passes(rnd(p1, "f32"), p1, bp)
    bad = O.adam(*args, bias_correction=False)[0]
    assert not passes(rnd(bad, "f32"), p1, bp)


@pytest.mark.parametrize("step", [1, 14])
def test_adam_tail_not_updated_rejected(adam_rec, step):
    ns = [n for n, _, _ in adam_rec["tensors"] if n % 4]
    assert ns, "no recorded tensor has an n % 4 tail"
    n = min(ns)
    args, p1, bp = _adam_case(adam_rec, n, step)
    bad = p1.copy()
    bad[n - n % 4:] = args[0][n - n % 4:]
    assert not passes(rnd(bad, "f32"), p1, bp)


# ---------------------------------------------------------------------------------------------------------------------
# flow up-sampler
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_flow_upsample_swapped_ky_parity_rejected(fmt):
    rec = _pick("ir2rgb_flow_upsample_slice")
    a = G.named_args(rec)
    g = _gen(9)
    x = rnd(torch.randn(1, 2, a["h"], a["w"], generator=g, dtype=torch.float64).numpy() * 4, "bf16")
    w = rnd(torch.randn(2, 2, 4, 4, generator=g, dtype=torch.float64).numpy() * 0.5, "bf16")
    bias = rnd(torch.randn(2, generator=g, dtype=torch.float64).numpy(), "bf16") if a["bias"] else None
    ref, S = O.flow_upsample(x, w, bias)
    bad, _ = O.flow_upsample(x, w, bias, swap_ky_parity=True)
    bnd = B.bound_sum(ref, S, fmt, 9)
    assert passes(rnd(ref, fmt), ref, bnd)
    assert not passes(rnd(bad, fmt), ref, bnd)


def test_flow_upsample_matches_conv_transpose():
    """The restatement agrees with torch's ConvTranspose2d(2, 2, 4, 2, 1) in fp64 (a check of the reference itself)."""
    g = _gen(10)
    x = torch.randn(2, 2, 5, 7, generator=g, dtype=torch.float64)
    w = torch.randn(2, 2, 4, 4, generator=g, dtype=torch.float64)
    b = torch.randn(2, generator=g, dtype=torch.float64)
    want = torch.nn.functional.conv_transpose2d(x, w, b, stride=2, padding=1).numpy()
    assert np.allclose(O.flow_upsample(x.numpy(), w.numpy(), b.numpy())[0], want, rtol=0, atol=1e-12)


def test_warp_blend_matches_grid_sample():
    """The restatement agrees with grid_sample(bilinear, border, align_corners=False) on the reference's grid."""
    g = _gen(11)
    N, H, W = 1, 9, 13
    raw = torch.randn(N, 3, H, W, generator=g, dtype=torch.float64)
    prev = torch.randn(N, 5, H, W, generator=g, dtype=torch.float64)
    flow = torch.randn(N, 2, H, W, generator=g, dtype=torch.float64) * 3
    w = torch.rand(N, 1, H, W, generator=g, dtype=torch.float64)
    gx = torch.linspace(-1, 1, W, dtype=torch.float64)[None, None, :] + flow[:, 0] / ((W - 1) / 2)
    gy = torch.linspace(-1, 1, H, dtype=torch.float64)[None, :, None] + flow[:, 1] / ((H - 1) / 2)
    warp = torch.nn.functional.grid_sample(prev[:, -3:], torch.stack([gx, gy], -1), mode="bilinear",
                                           padding_mode="border", align_corners=False)
    want = (raw * w + warp * (1 - w)).numpy()
    got = O.warp_blend(raw.numpy(), prev.numpy(), flow.numpy(), w.numpy())["out"]
    assert np.allclose(got, want, rtol=0, atol=1e-12)


def test_avgpool_matches_torch():
    g = _gen(12)
    for H, W in ((7, 10), (1, 6), (8, 1)):
        x = torch.randn(3, H, W, generator=g, dtype=torch.float64)
        want = torch.nn.functional.avg_pool2d(x[:, None], 3, 2, 1, count_include_pad=False)[:, 0].numpy()
        assert np.allclose(O.avgpool3s2(x.numpy())[0], want, rtol=0, atol=1e-12)
        xr = x.clone().requires_grad_(True)
        gy = torch.randn(want.shape, generator=g, dtype=torch.float64)
        torch.nn.functional.avg_pool2d(xr[:, None], 3, 2, 1, count_include_pad=False)[:, 0].backward(gy)
        assert np.allclose(O.avgpool3s2_bwd(gy.numpy(), H, W)[0], xr.grad.numpy(), rtol=0, atol=1e-12)
