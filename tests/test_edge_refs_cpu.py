"""The fp64 references of the edge records (oracle/edge_records.py) checked without a GPU.

oracle/window_ops_ref.py and oracle/bn_ref.py had only been exercised at the window's large shapes; at H <= 2 * pad,
one-pixel planes or N > 1 they could themselves be wrong.  At every edge record each reference is compared with an
independent torch fp64 formulation of the same operation (F.pad(reflect) and a sum over taps with autograd for the
adjoints, F.grid_sample, F.avg_pool2d, F.conv_transpose2d, F.unfold-style indexing, torch.optim.Adam, F.batch_norm in
training and evaluation mode): agreement to 1e-12 of the result's largest magnitude.  The conditions that keep the warp
records honest (a clamped pixel, few pixels in the ambiguity band) are checked on the reference alone; the planted
faults of tests/test_window_ops_bounds_cpu.py are shown to be rejected by the bounds at one edge record per family (a
bound that is tight at 512 x 1024 can be vacuous at 4 x 5); and every replayed entry and every BatchNorm entry point
must have an edge record.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import bn_ref as BR
from oracle import bounds as B
from oracle import conv_ref as R
from oracle import edge_records as E
from oracle import replay_kernels as K
from oracle import replay_ops as G
from oracle import window as WG
from oracle import window_ops_ref as O
from oracle.replay import gen, ids, passes, rnd

RTOL = 1e-12


def _recs(*entries):
    recs = [r for r in E.EDGE if r["entry"] in entries]
    return pytest.mark.parametrize("rec", recs, ids=ids(recs))


def _bn_recs(*entries):
    recs = [r for r in E.EDGE_BN if r["entry"] in entries]
    return pytest.mark.parametrize("rec", recs, ids=ids(recs))


def _close(got, want, what=""):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want.detach() if hasattr(want, "detach") else want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if got.size == 0:
        return
    scale = max(float(np.abs(want).max()), 1e-300)
    err = float(np.abs(got - want).max())
    assert err <= RTOL * scale, f"{what}: differs by {err:.3g} (largest magnitude {scale:.3g})"


def _rand(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale


def _act(pre, nb, mul):
    return torch.tanh(pre) if nb == 1 else (torch.sigmoid(pre) if nb == 2 else pre * mul)


# ---------------------------------------------------------------------------------------------------------------------
# completeness
def test_every_replayed_entry_has_an_edge_record():
    have = {r["entry"] for r in E.EDGE}
    assert not set(G.REPLAY) - have, sorted(set(G.REPLAY) - have)
    assert have <= set(G.REPLAY)
    assert len({WG.canon(r) for r in E.EDGE}) == len(E.EDGE), "a duplicate edge record"


def test_every_batchnorm_entry_point_has_an_edge_record():
    have = {r["entry"] for r in E.EDGE_BN}
    assert have == set(WG.BN_ENTRIES), sorted(have ^ set(WG.BN_ENTRIES))
    assert len({WG.canon(r) for r in E.EDGE_BN}) == len(E.EDGE_BN), "a duplicate edge record"
    bwd = [r["args"] for r in E.EDGE_BN if r["entry"] == "ir2rgb_bn_bwd"]
    for form in (0, 16, 32, 48):
        assert {a[12] & 15 for a in bwd if a[2] and a[12] & 48 == form} == {0, 1, 2}, form
    assert any(not a[2] for a in bwd)
    assert any(r["args"][16] for r in E.EDGE_BN if r["entry"] == "ir2rgb_bn_finalize_ex")
    assert {r["args"][15] for r in E.EDGE_BN if r["entry"] == "ir2rgb_bn_finalize_ex"} == {1, 2, 3}


def test_edge_records_are_not_window_records():
    """The edge tables add geometries; a record that repeats a manifest entry would add nothing."""
    man = {WG.canon(r) for r in WG.load()["launches"]}
    assert not [r for r in E.EDGE + E.EDGE_BN if WG.canon(r) in man]


def test_loss_records_are_what_the_kernel_accepts():
    """loss_pack's argument checks (losses.hip), and the block split the records are there for."""
    from ir2rgb_amd import _lib
    assert len(E.LOSS_ITEMS) == 32
    for items in (E.LOSS_ITEMS, E.LOSS_GAP):
        for it in items:
            assert it["n"] >= 1 and 0 <= it["slot"] <= 3
            if it["kind"] == 0:
                assert it["n"] % 8 == 0 and it["b"]
            if it["kind"] == 2:
                assert it["mask"] and it["hw"] >= 1 and it["chw"] % it["hw"] == 0 and it["n"] % it["chw"] == 0
    assert {it["kind"] for it in E.LOSS_ITEMS} == {0, 1, 2}
    assert any(it["kind"] == 2 and it["chw"] == it["hw"] for it in E.LOSS_ITEMS)
    assert any(it["kind"] == 2 and it["n"] == 3 * it["chw"] for it in E.LOSS_ITEMS)
    assert any(it["kind"] == 2 and not it["b"] for it in E.LOSS_ITEMS)
    ns = [it["n"] for it in E.LOSS_ITEMS]
    nb = [min(int((G.LOSS_BLOCKS - len(ns)) * n / float(sum(ns))) + 1, -(-n // 2048)) for n in ns]
    assert sum(nb) <= G.LOSS_BLOCKS and max(nb) > 100 and nb[ns.index(2056)] == 2
    assert all(b == 1 for n, b in zip(ns, nb) if n <= 2048)
    assert sorted({it["slot"] for it in E.LOSS_GAP}) == [0, 2]
    assert "ir2rgb_loss_multi_fwd" in _lib.PROTOTYPES


# ---------------------------------------------------------------------------------------------------------------------
# heads
def _head_torch(T, bias, Cout, KH, pad, acts, mul):
    """F.pad(reflect) and a sum over taps: T [N,H,W,CT] -> out [N,Cout,H,W]."""
    H = T.shape[1]
    Tp = F.pad(T.permute(0, 3, 1, 2), (0, 0, pad, pad), mode="reflect") if pad else T.permute(0, 3, 1, 2)
    outs = []
    for co in range(Cout):
        pre = sum(Tp[:, co * KH + ky, ky:ky + H] for ky in range(KH))
        if bias is not None:
            pre = pre + bias[co]
        outs.append(_act(pre, O.nibble(acts, co), mul))
    return torch.stack(outs, 1)


@_recs("ir2rgb_head_finish", "ir2rgb_head_finish_bwd")
def test_head_reference_matches_reflect_pad_and_autograd(rec):
    a = G.named_args(rec)
    N, H, W, Cout, KH, CT, pad, acts, mul = (a[k] for k in "N H W Cout KH CT pad_h acts mul".split())
    g = gen(rec)
    T = _rand(g, N, H, W, CT, scale=0.5).requires_grad_(True)
    bias = _rand(g, Cout, scale=0.5).requires_grad_(True)
    use_bias = a.get("bias", True)
    out = _head_torch(T, bias if use_bias else None, Cout, KH, pad, acts, mul)
    ref, _, _ = O.head_finish(T.detach().numpy(), bias.detach().numpy() if use_bias else None, Cout, KH, pad, acts, mul)
    _close(ref, out, "head_finish")
    gout = _rand(g, N, Cout, H, W)
    out.backward(gout)
    dT, dbias, _, _ = O.head_finish_bwd(gout.numpy(), out.detach().numpy(), Cout, KH, CT, pad, acts, mul)
    _close(dT, T.grad, "head_finish_bwd dT")
    assert not dT[..., Cout * KH:].any()
    if use_bias:
        _close(dbias, bias.grad, "head_finish_bwd dbias")


# ---------------------------------------------------------------------------------------------------------------------
# warp_blend
def _warp_rec_inputs(rec):
    a = G.named_args(rec)
    N, Cp, H, W = a["N"], a["Cp"], a["H"], a["W"]
    g = gen(rec)
    raw, prev, flow, w = G._warp_inputs(N, Cp, H, W, g)
    return a, g, [t.double() for t in (raw, prev, flow, w)]


@_recs("ir2rgb_warp_blend_fwd", "ir2rgb_warp_blend_bwd")
def test_warp_record_has_clamped_pixels_and_a_thin_ambiguity_band(rec):
    """On the fp64 reference alone: replay_warp_bwd's clamped.sum() > 0 holds, and at most 10 % of the pixels lie
    where the cell or the clamp is a matter of the last bit of the coordinate."""
    a, g, (raw, prev, flow, w) = _warp_rec_inputs(rec)
    H, W = a["H"], a["W"]
    r = O.warp_blend(raw.numpy(), prev.numpy(), flow.numpy(), w.numpy())
    clamped = ~((r["ix"] > 0) & (r["ix"] < W - 1))
    assert clamped.sum() > 0
    amb = G._ambiguous(r, H, W)
    assert amb.mean() <= 0.10, f"{int(amb.sum())} of {amb.size} pixels in the ambiguity band"
    assert (~clamped).sum() > 0, "every pixel is clamped in x: the flow gradient in x is never exercised"


@_recs("ir2rgb_warp_blend_fwd", "ir2rgb_warp_blend_bwd")
def test_warp_reference_matches_grid_sample(rec):
    a, g, (raw, prev, flow, w) = _warp_rec_inputs(rec)
    N, H, W = a["N"], a["H"], a["W"]
    raw, flow, w = raw.requires_grad_(True), flow.requires_grad_(True), w.requires_grad_(True)
    gx = torch.linspace(-1, 1, W, dtype=torch.float64)[None, None, :] + flow[:, 0] / ((W - 1) / 2)
    gy = torch.linspace(-1, 1, H, dtype=torch.float64)[None, :, None] + flow[:, 1] / ((H - 1) / 2)
    warp = F.grid_sample(prev[:, -3:], torch.stack([gx, gy], -1), mode="bilinear", padding_mode="border", align_corners=False)
    out = raw * w + warp * (1 - w)
    gout = _rand(g, N, 3, H, W)
    r = O.warp_blend(raw.detach().numpy(), prev.numpy(), flow.detach().numpy(), w.detach().numpy(), gout=gout.numpy())
    _close(r["warp"], warp, "warp")
    _close(r["out"], out, "out")
    out.backward(gout)
    _close(r["graw"], raw.grad, "graw")
    _close(r["gw"], w.grad, "gw")
    amb = np.broadcast_to(G._ambiguous(r, H, W)[:, None], r["gflow"].shape)
    _close(np.where(amb, 0, r["gflow"]), torch.where(torch.from_numpy(amb.copy()), torch.zeros(()).double(), flow.grad), "gflow")


@_recs("ir2rgb_warp_diff_norm_fwd")
def test_resample_reference_matches_grid_sample(rec):
    """resample2d (corners clamped, weights from the unclamped fraction) equals grid_sample(align_corners=True, border):
    beyond the border both corners clamp onto the edge pixel, whatever the weights."""
    a = G.named_args(rec)
    N, C, H, W = a["N"], a["C"], a["H"], a["W"]
    g = gen(rec)
    img1, img2 = _rand(g, N, C, H, W), _rand(g, N, C, H, W)
    flow = G._pixel_flow(N, H, W, g).double()
    v, _, _, _ = O.resample2d(img2.numpy(), flow.numpy())
    xs = torch.arange(W, dtype=torch.float64)[None, None, :] + flow[:, 0]
    ys = torch.arange(H, dtype=torch.float64)[None, :, None] + flow[:, 1]
    # align_corners=True: pixel i <-> -1 + 2 i / (n - 1); a one-pixel axis has a single sample whatever the coordinate
    nx = xs * (2.0 / (W - 1)) - 1 if W > 1 else torch.zeros_like(xs)
    ny = ys * (2.0 / (H - 1)) - 1 if H > 1 else torch.zeros_like(ys)
    want = F.grid_sample(img2, torch.stack([nx.expand(N, H, W), ny.expand(N, H, W)], -1), mode="bilinear",
                         padding_mode="border", align_corners=True)
    err = np.abs(v - want.numpy()).max()
    assert err <= RTOL * max(1.0, float(want.abs().max())), err
    d = img1.numpy() - v
    _close(np.sqrt((d * d).sum(1, keepdims=True)), torch.linalg.vector_norm(torch.from_numpy(d), dim=1, keepdim=True), "norm")


# ---------------------------------------------------------------------------------------------------------------------
# pooling, up-sampler, xexpand, fold
@_recs("ir2rgb_avgpool3s2")
def test_avgpool_reference_matches_torch(rec):
    a = G.named_args(rec)
    P, H, W = a["planes"], a["H"], a["W"]
    g = gen(rec)
    x = _rand(g, P, H, W).requires_grad_(True)
    y = F.avg_pool2d(x[:, None], 3, 2, 1, count_include_pad=False)[:, 0]
    _close(O.avgpool3s2(x.detach().numpy())[0], y, "avgpool")
    gy = _rand(g, *y.shape)
    y.backward(gy)
    _close(O.avgpool3s2_bwd(gy.numpy(), H, W)[0], x.grad, "avgpool_bwd")


@_recs("ir2rgb_flow_upsample_slice")
def test_flow_upsample_reference_matches_conv_transpose(rec):
    a = G.named_args(rec)
    g = gen(rec)
    x, w, b = _rand(g, a["N"], 2, a["h"], a["w"], scale=4), _rand(g, 2, 2, 4, 4, scale=0.5), _rand(g, 2)
    bias = b if a["bias"] else None
    want = F.conv_transpose2d(x, w, bias, stride=2, padding=1)
    _close(O.flow_upsample(x.numpy(), w.numpy(), None if bias is None else b.numpy())[0], want, "flow_upsample")


def _xexpand_torch(x, Wout, KW, s, p, pm, Cx):
    """F.pad and F.unfold: x [N,Cin,H,W] -> [N,H,Wout,Cx]."""
    N, Cin, H, W = x.shape
    xp = F.pad(x, (p, p, 0, 0), mode="reflect" if pm else "constant") if p else x
    cols = F.unfold(xp.reshape(N * Cin * H, 1, 1, W + 2 * p), (1, KW), stride=(1, s))       # [N*Cin*H, KW, L]
    cols = cols[:, :, :Wout].reshape(N, Cin, H, KW, Wout).permute(0, 2, 4, 1, 3).reshape(N, H, Wout, Cin * KW)
    return F.pad(cols, (0, Cx - Cin * KW))


@_recs("ir2rgb_xexpand", "ir2rgb_xexpand_cx", "ir2rgb_xexpand_bwd")
def test_xexpand_reference_matches_unfold_and_autograd(rec):
    a = G.named_args(rec)
    N, Cin, H, W, Wout, KW, s, p, pm = (a[k] for k in "N Cin H W Wout KW stride_w pad_w pad_mode".split())
    Cx = a.get("Cx", 64)
    assert Wout == (W + 2 * p - KW) // s + 1 and Cin * KW <= Cx and (not pm or p < W)
    g = gen(rec)
    x = _rand(g, N, Cin, H, W).requires_grad_(True)
    want = _xexpand_torch(x, Wout, KW, s, p, pm, Cx)
    _close(O.xexpand(x.detach().numpy(), Wout, KW, s, p, pm, Cx), want, "xexpand")
    dxe = _rand(g, N, H, Wout, Cx)
    want.backward(dxe)
    _close(O.xexpand_bwd(dxe.numpy(), Cin, W, KW, s, p, pm)[0], x.grad, "xexpand_bwd")


@_recs("ir2rgb_fold_reflect")
def test_fold_reference_is_the_adjoint_of_reflection_pad(rec):
    a = G.named_args(rec)
    N, H, W, C, ph, pw = (a[k] for k in "N H W C pad_h pad_w".split())
    g = gen(rec)
    x = _rand(g, N, C, H, W).requires_grad_(True)
    xp = F.pad(x, (pw, pw, ph, ph), mode="reflect")
    dxpad = _rand(g, N, C, H + 2 * ph, W + 2 * pw)
    xp.backward(dxpad)
    dx, cnt = O.fold_reflect(dxpad.permute(0, 2, 3, 1).numpy(), ph, pw)
    _close(dx, x.grad.permute(0, 2, 3, 1), "fold_reflect")
    assert cnt.sum() == (H + 2 * ph) * (W + 2 * pw)


# ---------------------------------------------------------------------------------------------------------------------
# losses and Adam
@_recs("ir2rgb_loss_multi_fwd", "ir2rgb_loss_multi_bwd")
def test_loss_reference_matches_torch(rec):
    g = gen(rec)
    for it in rec["items"]:
        n = it["n"]
        a = _rand(g, n).requires_grad_(True)
        b = _rand(g, n) if it["b"] else None
        if it["kind"] == 0:
            loss, mask = (a - b).abs().mean(), None
        elif it["kind"] == 1:
            loss, mask = ((a - it["target"]) ** 2).mean(), None
        else:
            Nn, Cc = n // it["chw"], it["chw"] // it["hw"]
            mask = torch.rand(Nn, 1, it["hw"], generator=g, dtype=torch.float64)
            av = a.view(Nn, Cc, it["hw"])
            bv = b.view(Nn, Cc, it["hw"]) if b is not None else torch.zeros_like(av)
            loss = (av * mask - bv * mask).abs().mean()
        an, bn, mn = a.detach().numpy(), None if b is None else b.numpy(), None if mask is None else mask.numpy()
        term, _ = O.loss_term(it["kind"], an, bn, mn, it["target"], it["hw"], it["chw"])
        _close(np.array(term.sum() / n), loss, f"loss kind {it['kind']} n {n}")
        (loss * it["weight"]).backward()
        _close(O.loss_grad(it["kind"], an, bn, mn, it["target"], it["hw"], it["chw"], it["weight"] / n), a.grad,
               f"loss gradient kind {it['kind']} n {n}")


@pytest.mark.parametrize("step", [1, 14])
def test_adam_reference_matches_torch_optim(step):
    rec = E.ADAM
    g = gen(rec)
    b1, b2 = float(np.float32(rec["beta1"])), float(np.float32(rec["beta2"]))
    for n in sorted({n for n, _, _ in rec["tensors"]}):
        p, gr = _rand(g, n, scale=0.05), _rand(g, n, scale=0.01)
        m = torch.zeros(n, dtype=torch.float64) if step == 1 else _rand(g, n, scale=0.01)
        v = torch.zeros(n, dtype=torch.float64) if step == 1 else torch.rand(n, generator=g, dtype=torch.float64) * 1e-4
        ref = O.adam(p.numpy(), gr.numpy(), m.numpy(), v.numpy(), rec["lr"], b1, b2, rec["eps"], step)
        q = p.clone().requires_grad_(True)
        opt = torch.optim.Adam([q], lr=rec["lr"], betas=(b1, b2), eps=rec["eps"], foreach=False)
        if step > 1:
            opt.state[q] = {"step": torch.tensor(float(step - 1)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
        q.grad = gr.clone()
        opt.step()
        _close(ref[0], q, f"adam p (n {n})")
        _close(ref[1], opt.state[q]["exp_avg"], "adam m")
        _close(ref[2], opt.state[q]["exp_avg_sq"], "adam v")


# ---------------------------------------------------------------------------------------------------------------------
# BatchNorm
def _bn_act(z, act):
    return torch.relu(z) if act == 1 else (F.leaky_relu(z, 0.2) if act == 2 else z)


def _bn_inputs(rec, P, C):
    g = gen(rec)
    y = K._bn_data(P, C, g).double()
    vec = [K._vec(C, g, 0.5, 1.5).double(), K._vec(C, g).double(), (K._vec(C, g) * 0.2).double(), K._vec(C, g).double(),
           K._vec(C, g, 0.5, 2.0).double()]
    return g, y, vec        # gamma, beta, conv_bias, running_mean, running_var


@_bn_recs("ir2rgb_bn_finalize", "ir2rgb_bn_finalize_ex", "ir2rgb_bn_finalize_apply")
def test_bn_finalize_reference_matches_batch_norm(rec):
    a = rec["args"]
    if rec["entry"] == "ir2rgb_bn_finalize":
        a = a[:6] + [False] + a[6:] + [0]
    rows_n, C, P, mom, eps, upd = a[1], a[2], a[3], a[9], a[10], a[15]
    frozen = rec["entry"] == "ir2rgb_bn_finalize_ex" and a[16]
    act = a[21] if rec["entry"] == "ir2rgb_bn_finalize_apply" else 0
    g, y, (gamma, beta, cb, rm, rv) = _bn_inputs(rec, P, C)
    if not a[6]:
        cb = torch.zeros_like(cb)
    res = [_rand(g, P, C) if rec["entry"] == "ir2rgb_bn_finalize_apply" and a[17 + i] else None for i in range(2)]
    rows = torch.stack([torch.stack([c.sum(0), (c * c).sum(0)]) for c in torch.tensor_split(y, rows_n)]).numpy()
    vn = [t.numpy() for t in (gamma, beta, cb, rm, rv)]
    rm_t, rv_t = rm.clone(), rv.clone()
    if frozen:
        ref = BR.finalize_frozen(*vn, eps)
        want = F.batch_norm(y + cb, rm_t, rv_t, gamma, beta, False, mom, eps)
    elif P == 1:
        # nn.BatchNorm2d refuses one value per channel in training mode: the definition itself, with the biased variance
        ref = BR.finalize(rows, float(P), *vn, mom, eps, upd)
        want = beta.expand(1, C)
        keep = (1 - mom) ** upd
        _close(ref["running_var"][0], keep * rv, "running_var at count 1")
        _close(ref["running_mean"][0], keep * rm + (1 - keep) * (y[0] + cb), "running_mean at count 1")
    else:
        ref = BR.finalize(rows, float(P), *vn, mom, eps, upd)
        for _ in range(upd):
            want = F.batch_norm(y + cb, rm_t, rv_t, gamma, beta, True, mom, eps)
        _close(ref["running_mean"][0], rm_t, "running_mean")
        _close(ref["running_var"][0], rv_t, "running_var")
    rr = [r.numpy() if r is not None else None for r in res]
    z, _ = BR.apply(y.numpy(), ref["scale"][0], ref["shift"][0], act, rr[0], rr[1], "bf16")
    want = _bn_act(want, act)
    for r in res:
        if r is not None:
            want = want + r
    # (E[y^2] - E[y]^2 against torch's centred variance: the cancellation costs |mean|^2 / var of the last bits)
    err = np.abs(z - want.numpy()).max()
    assert err <= RTOL * max(1.0, float(want.abs().max())), err
    assert all(np.all(np.isfinite(b)) and np.all(np.asarray(b) >= 0) for _, b in ref.values())


@_bn_recs("ir2rgb_bn_apply")
def test_bn_apply_reference_matches_eval_batch_norm(rec):
    a = rec["args"]
    P, C, act = a[6], a[7], a[8]
    g, y, (gamma, beta, cb, rm, rv) = _bn_inputs(rec, P, C)
    res = [_rand(g, P, C) if a[3 + i] else None for i in range(2)]
    ref = BR.finalize_frozen(*(t.numpy() for t in (gamma, beta, cb, rm, rv)), 1e-5)
    want = _bn_act(F.batch_norm(y + cb, rm, rv, gamma, beta, False, 0.1, 1e-5), act)
    for r in res:
        if r is not None:
            want = want + r
    z, bnd = BR.apply(y.numpy(), ref["scale"][0], ref["shift"][0], act, *[r.numpy() if r is not None else None for r in res], "f16")
    _close(z, want, "bn_apply")
    assert (bnd > 0).all()


@_bn_recs("ir2rgb_bn_bwd")
def test_bn_bwd_reference_matches_autograd(rec):
    a = rec["args"]
    P, C, act, has_scale = a[10], a[11], a[12], a[2]
    frozen, acc, act = bool(act & 16), bool(act & 32), act & 15
    g, y, (gamma, beta, _, rm, rv) = _bn_inputs(rec, P, C)
    eps = 1e-5
    gz = _rand(g, P, C)
    base = (_rand(g, C), _rand(g, C)) if acc else None
    x = y.clone().requires_grad_(True)
    if not has_scale:
        bias = torch.zeros(C, dtype=torch.float64, requires_grad=True)
        # (the activation's kink: y itself is the pre-activation, and a convolution's bias moves all of a channel alike)
        _bn_act(x + bias, act).backward(gz)
        ref = BR.bwd(gz.numpy(), y.numpy(), None, None, None, None, act, "bf16",
                     None if base is None else (base[0].numpy(), base[1].numpy()))
        _close(ref["gy"][0], x.grad, "gy")
        _close(ref["dbeta"][0], bias.grad + (base[1] if acc else 0), "dbeta")
        return
    gm, bt = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    if frozen:
        mean, invstd = rm, 1.0 / torch.sqrt(rv + eps)
        z = F.batch_norm(x, rm, rv, gm, bt, False, 0.1, eps)
    elif P == 1:
        # one value per channel: yhat = 0 and gy = 0 by the definition; torch refuses the case
        mean, invstd = y[0], torch.full((C,), 1.0 / np.sqrt(eps), dtype=torch.float64)
        z = None
    else:
        mean, invstd = y.mean(0), 1.0 / torch.sqrt(y.var(0, unbiased=False) + eps)
        z = F.batch_norm(x, None, None, gm, bt, True, 0.1, eps)
    scale = gamma * invstd
    shift = beta - mean * scale
    ref = BR.bwd(gz.numpy(), y.numpy(), scale.numpy(), shift.numpy(), mean.numpy(), invstd.numpy(), act, "bf16",
                 None if base is None else (base[0].numpy(), base[1].numpy()), frozen=frozen)
    if z is None:
        gp = gz * torch.from_numpy(BR.dact_np((y * scale + shift).numpy(), act))
        _close(ref["dbeta"][0], gp.sum(0) + (base[1] if acc else 0), "dbeta at one pixel")
        assert np.abs(ref["gy"][0]).max() <= 1e-9 * float((scale.abs() * gp.abs()).max() + 1e-300)
        return
    _bn_act(z, act).backward(gz)
    # (gy of training mode is a difference of terms n times its size: relative to their magnitude, as the bound is)
    mag = float((scale.abs() * (gz.abs().max(0).values + gz.abs().sum(0) / P * (1 + ((y - mean) * invstd).abs().max(0).values))).max())
    assert np.abs(ref["gy"][0] - x.grad.numpy()).max() <= RTOL * mag
    S = float(gz.abs().sum(0).max()) * max(1.0, float(((y - mean) * invstd).abs().max()))
    assert np.abs(ref["dbeta"][0] - (bt.grad + (base[1] if acc else 0)).numpy()).max() <= RTOL * S
    assert np.abs(ref["dgamma"][0] - (gm.grad + (base[0] if acc else 0)).numpy()).max() <= RTOL * S


# ---------------------------------------------------------------------------------------------------------------------
# the planted faults of test_window_ops_bounds_cpu.py at an edge record of each family
def _edge(entry, **want):
    for r in E.EDGE:
        if r["entry"] == entry and all(G.named_args(r)[k] == v for k, v in want.items()):
            return r
    raise LookupError((entry, want))


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("H", [4, 7, 13])
@pytest.mark.parametrize("edge", ["top", "bottom"])
def test_head_finish_bwd_missing_mirror_rejected_at_edge_record(fmt, H, edge):
    """pad < H <= 2 * pad: the mirror of one border lands next to the other one.  One mirror contribution dropped."""
    rec = _edge("ir2rgb_head_finish_bwd", H=H, W=5)
    a = G.named_args(rec)
    g = gen(rec)
    shape = (a["N"], a["Cout"], H, a["W"])
    pre = _rand(g, *shape, scale=2)
    out = rnd(torch.stack([_act(pre[:, co], O.nibble(a["acts"], co), a["mul"]) for co in range(a["Cout"])], 1).numpy(), "f32")
    gout = rnd(_rand(g, *shape).numpy(), "f32")
    dT, _, S, _ = O.head_finish_bwd(gout, out, a["Cout"], a["KH"], a["CT"], a["pad_h"], a["acts"], a["mul"])
    bnd = B.bound_rw(dT, S, fmt, 3, 6)
    assert passes(rnd(dT, fmt), dT, bnd)
    y = 0 if edge == "top" else H - 1
    ky = 0 if edge == "top" else a["KH"] - 1
    dst = int(O.refl(np.array([y + ky - a["pad_h"]]), H)[0])
    assert dst != y
    nb = O.nibble(a["acts"], 0)
    o, gg = out[:, 0, y], gout[:, 0, y]
    bad = dT.copy()
    bad[:, dst, :, ky] -= gg * (1 - o * o) if nb == 1 else (gg * o * (1 - o) if nb == 2 else gg * a["mul"])
    assert not passes(rnd(bad, fmt), dT, bnd)


@pytest.mark.parametrize("H", [4, 9])
def test_head_finish_dropped_mirror_rejected_at_edge_record(H):
    """The forward with the bottom mirror replaced by an edge repeat (clamp instead of reflect)."""
    rec = _edge("ir2rgb_head_finish", H=H, W=5)
    a = G.named_args(rec)
    g = gen(rec)
    T = _rand(g, a["N"], H, a["W"], a["CT"], scale=0.5).numpy()
    bias = _rand(g, a["Cout"], scale=0.5).numpy()
    out, pre, S = O.head_finish(T, bias, a["Cout"], a["KH"], a["pad_h"], a["acts"], a["mul"])
    bnd = B.bound_act(out, O.act_slope(out, a["acts"], a["mul"], a["Cout"]), S, a["KH"] + 1)
    assert passes(rnd(out, "f32"), out, bnd)
    Tc = np.concatenate([T, np.repeat(T[:, -1:], a["pad_h"], 1)], 1)       # rows beyond H - 1 repeat the last row
    pre_bad = pre.copy()
    for co in range(a["Cout"]):
        for ky in range(a["KH"]):
            t = H - 1 + ky - a["pad_h"]
            if t > H - 1:
                pre_bad[:, co, H - 1] += Tc[:, t, :, co * a["KH"] + ky] - T[:, O.refl(np.array([t]), H)[0], :, co * a["KH"] + ky]
    bad = np.stack([_act(torch.from_numpy(pre_bad[:, co]), O.nibble(a["acts"], co), a["mul"]).numpy() for co in range(a["Cout"])], 1)
    assert not passes(rnd(bad, "f32"), out, bnd)


@pytest.mark.parametrize("backward", [0, 1])
@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 1, 7), (5, 2, 2)])
def test_avgpool_count_include_pad_rejected_at_edge_record(backward, shape):
    rec = _edge("ir2rgb_avgpool3s2", planes=shape[0], H=shape[1], W=shape[2], backward=backward)
    P, H, W = shape
    g = gen(rec)
    if not backward:
        x = rnd(_rand(g, P, H, W).numpy(), "f32")
        (ref, S), (bad, _) = O.avgpool3s2(x), O.avgpool3s2(x, count_include_pad=True)
        bnd = B.bound_sum(ref, S, "f32", 10)
    else:
        gy = rnd(_rand(g, P, (H - 1) // 2 + 1, (W - 1) // 2 + 1).numpy(), "f32")
        (ref, S), (bad, _) = O.avgpool3s2_bwd(gy, H, W), O.avgpool3s2_bwd(gy, H, W, count_include_pad=True)
        bnd = B.bound_sum(ref, S, "f32", 8)
    assert passes(rnd(ref, "f32"), ref, bnd)
    assert not passes(rnd(bad, "f32"), ref, bnd)


@pytest.mark.parametrize("step", [1, 14])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 8191, 8193, 16387])
def test_adam_tail_not_updated_rejected_at_edge_record(step, n):
    rec = E.ADAM
    assert n % 4 and [n, True, 1] in rec["tensors"] and [n, False, 1] in rec["tensors"]
    g = gen(rec)
    p = rnd(_rand(g, n, scale=0.05).numpy(), "f32")
    gr = rnd(_rand(g, n, scale=0.01).numpy(), "f32")
    m = np.zeros(n) if step == 1 else rnd(_rand(g, n, scale=0.01).numpy(), "f32")
    v = np.zeros(n) if step == 1 else rnd((torch.rand(n, generator=g, dtype=torch.float64) * 1e-4).numpy(), "f32")
    b1, b2 = float(np.float32(rec["beta1"])), float(np.float32(rec["beta2"]))
    p1, m1, v1, upd, Sm, ss, den = O.adam(p, gr, m, v, rec["lr"], b1, b2, rec["eps"], step)
    bm = 4 * B.U32 * Sm + B.ETA["f32"]
    bp = B.U32 * np.abs(p1) + 16 * B.U32 * upd + ss * bm / den + B.ETA["f32"]
    assert passes(rnd(p1, "f32"), p1, bp)
    bad = p1.copy()
    bad[n - n % 4:] = p[n - n % 4:]
    assert not passes(rnd(bad, "f32"), p1, bp)
    bad_m = m1.copy()
    bad_m[n - n % 4:] = m[n - n % 4:]
    assert not passes(rnd(bad_m, "f32"), m1, bm)


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_bn_bwd_frozen_as_training_rejected_at_edge_record(fmt):
    """Evaluation mode answered with the training-mode gradient (the mean / variance terms left in), at 2 and 513 pixels."""
    for rec in [r for r in E.EDGE_BN if r["entry"] == "ir2rgb_bn_bwd" and r["args"][12] & 16 and r["args"][10] in (2, 513)]:
        a = rec["args"]
        P, C, act = a[10], a[11], a[12] & 15
        g, y, (gamma, beta, _, rm, rv) = _bn_inputs(rec, P, C)
        gz = R.draw((P, C), g).double().numpy()
        invstd = (1.0 / torch.sqrt(rv + 1e-5)).numpy()
        scale = gamma.numpy() * invstd
        shift = beta.numpy() - rm.numpy() * scale
        gz[~BR.sign_safe(y.numpy(), scale, shift)] = 0
        good = BR.bwd(gz, y.numpy(), scale, shift, rm.numpy(), invstd, act, fmt, frozen=True)
        bad = BR.bwd(gz, y.numpy(), scale, shift, rm.numpy(), invstd, act, fmt)
        assert not BR.rejects(rnd(good["gy"][0], fmt), good["gy"])
        assert BR.rejects(rnd(bad["gy"][0], fmt), good["gy"]), (P, C, act)
