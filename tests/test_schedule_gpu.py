"""GPU side of the training schedule: the finest-scale-only epochs against the full trainer (tolerance 0) and against a
golden made by the reference's own code, ``update_fixed_params``, the learning rate through the optimizer kernels, the
device loss log (csrc/loss_log.hip) and ``ir2rgb_amd.training.fit`` end to end.

Everything runs at 64x128 with two spatial scales and tests/golden/window_stub.stub_flow_and_conf as the flow network.
Training is bit-reproducible, so trainer-against-trainer comparisons are exact: a difference is a finding.
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
from window_stub import stub_flow_and_conf  # noqa: E402

DTYPES = [torch.float16, torch.bfloat16]
SEQ_TOL = {torch.float16: 3e-2, torch.bfloat16: 6e-2}        # (tests/test_harness_gpu.py)


def bits(t):
    """The tensor's bytes (so that NaN equals NaN and -0.0 differs from 0.0)."""
    return t.detach().reshape(-1).contiguous().view(torch.uint8)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def trainer(dev, dtype, **kw):
    from ir2rgb_amd import vid2vid as V
    kw.setdefault("first_layer_gen_filters", 32)
    tr = V.Vid2VidTrainer(dev, compute_dtype=dtype, n_scales_spatial=2, build_flow_net=False, **kw)
    tr.flow_net = stub_flow_and_conf
    return tr


def snapshot(module):
    return {k: v.detach().clone() for k, v in module.state_dict().items()}


def params_of(module):
    return {k: v.detach().clone() for k, v in module.named_parameters()}


@pytest.fixture(scope="module")
def sequence(dev):
    from ir2rgb_amd import vid2vid as V
    return V.synthetic_sequence(6, 64, 128, 3, dev)


# ---------------------------------------------------------------------------------------------
# finest-scale-only epochs
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_fix_global_against_the_full_trainer(dev, sequence, dtype):
    A, B = sequence
    full, fix = trainer(dev, dtype), trainer(dev, dtype, niter_fix_global=1)
    assert full.finetune_all and not fix.finetune_all
    coarse0 = params_of(fix.netG[0])
    fine0 = params_of(fix.netG[1])
    coarse_ids = {id(p) for p in fix.netG[0].parameters()}
    assert not coarse_ids & {id(p) for p in fix.optimizer_G.params} and not coarse_ids & {id(p) for p in fix.grads_G.params}
    assert {id(p) for p in fix.optimizer_G.params} == {id(p) for p in fix.netG[1].parameters()}
    assert fix.optimizer_G.exp_avg.numel() == sum(p.numel() for p in fix.netG[1].parameters())
    out_full, out_fix = full.train_window(A[:, 0:3], B[:, 0:3]), fix.train_window(A[:, 0:3], B[:, 0:3])
    assert set(out_full) == set(out_fix)
    diff = [k for k in out_full if not same(out_full[k], out_fix[k])]
    assert not diff, {k: (out_full[k].item(), out_fix[k].item()) for k in diff}
    for name, a, b in zip(("fake_B", "fake_B_raw", "flow", "weight"), full.last_outputs, fix.last_outputs):
        assert same(a, b), name
    sa, sb = full.netG[1].state_dict(), fix.netG[1].state_dict()
    assert not [k for k in sa if not same(sa[k], sb[k])], "finest-scale parameters / buffers differ"
    for a, b in zip([full.netD] + full.netD_T, [fix.netD] + fix.netD_T):
        assert all(same(x, y) for x, y in zip(a.state_dict().values(), b.state_dict().values()))
    ba, bb = dict(full.netG[0].named_buffers()), dict(fix.netG[0].named_buffers())
    running = [k for k in ba if "running" in k]
    assert running and all(same(ba[k], bb[k]) for k in running), "coarse running statistics differ"
    assert any(not same(ba[k], torch.zeros_like(ba[k])) for k in running if "mean" in k), "running means never advanced"

    def coarse_untouched():
        for k, p in fix.netG[0].named_parameters():
            assert p.grad is None, k
            assert same(p, coarse0[k]), k

    coarse_untouched()
    assert any(not same(p, coarse0[k]) for k, p in full.netG[0].named_parameters()), "the full trainer's coarse scale did not train"
    for i in (1, 2):
        fix.train_window(A[:, i:i + 3], B[:, i:i + 3])
    coarse_untouched()
    moved = [k for k, p in fix.netG[1].named_parameters() if not same(p, fine0[k])]
    assert len(moved) > len(fine0) // 2, "the finest scale did not train"


def _load_from(fresh, tr):
    for a, b in zip(fresh.netG + [fresh.netD] + fresh.netD_T, tr.netG + [tr.netD] + tr.netD_T):
        a.load_state_dict(b.state_dict())
    # the discriminators' optimizers carry on (update_fixed_params replaces the generator's only)
    for a, b in zip([fresh.optimizer_D] + fresh.optimizer_D_T, [tr.optimizer_D] + tr.optimizer_D_T):
        a.load_state_dict(b.state_dict())
    fresh.optimizer_G.param_groups[0]["lr"] = tr.optimizer_G.param_groups[0]["lr"]
    if tr.loss_scaler is not None:
        fresh.loss_scaler.load_state_dict(tr.loss_scaler.state_dict())


@pytest.mark.parametrize("dtype,loss_scale", [(torch.bfloat16, None), (torch.float16, None), (torch.float16, "dynamic")])
def test_update_fixed_params(dev, sequence, dtype, loss_scale):
    A, B = sequence
    fix = trainer(dev, dtype, niter_fix_global=1, loss_scale=loss_scale)
    fix.train_window(A[:, 0:3], B[:, 0:3])
    old_grads, old_opt = fix.grads_G, fix.optimizer_G
    lr = fix.optimizer_G.param_groups[0]["lr"]
    fix.update_fixed_params()
    assert fix.finetune_all and fix.optimizer_G is not old_opt and fix.grads_G is not old_grads
    every = [p for g in fix.netG for p in g.parameters()]
    assert [id(p) for p in fix.optimizer_G.params] == [id(p) for p in every] == [id(p) for p in fix.grads_G.params]
    assert fix.optimizer_G.step_count == 0 and not fix.optimizer_G.exp_avg.any() and not fix.optimizer_G.exp_avg_sq.any()
    assert fix.optimizer_G.param_groups[0]["lr"] == lr == 2e-4
    assert all(p.grad is None for p in every) and not old_grads._hooks and not old_grads.direct
    if loss_scale is not None:      # the tables are those of the new optimizer set
        keys = list(fix.loss_scaler._tables)
        assert len(keys) == fix.t_scales + 1 and all(k[0] == id(fix.optimizer_G) for k in keys)
        state = fix.optimizer_G.scaled_state().data_ptr()
        assert all(int(t[0].item()) == state for t in fix.loss_scaler._tables.values())
    fresh = trainer(dev, dtype, loss_scale=loss_scale)
    _load_from(fresh, fix)
    coarse = params_of(fix.netG[0])
    fix.reset_sequence(), fresh.reset_sequence()
    out_a, out_b = fix.train_window(A[:, 1:4], B[:, 1:4]), fresh.train_window(A[:, 1:4], B[:, 1:4])
    assert set(out_a) == set(out_b) and not [k for k in out_a if not same(out_a[k], out_b[k])]
    for a, b in zip(fix.netG + [fix.netD] + fix.netD_T, fresh.netG + [fresh.netD] + fresh.netD_T):
        sa, sb = a.state_dict(), b.state_dict()
        assert not [k for k in sa if not same(sa[k], sb[k])]
    skipped = 0
    if loss_scale is not None:
        sa, sb = fix.loss_scaler.stats(), fresh.loss_scaler.stats()
        assert sa["scale"] == sb["scale"] and sa["skipped"] == sb["skipped"]
        skipped = fix.optimizer_G.grad_stats()[0]
    if not skipped:             # (a window whose scaled gradient overflowed moves nothing, on either side)
        assert any(not same(p, coarse[k]) for k, p in fix.netG[0].named_parameters()), "the coarse scale does not train"
    opt_now = fix.optimizer_G
    fix.update_fixed_params()   # a second call changes nothing
    assert fix.optimizer_G is opt_now


# ---------------------------------------------------------------------------------------------
# against the reference (tests/golden/make_schedule_goldens.py)
# ---------------------------------------------------------------------------------------------
def _seeded(g, dev, dtype):
    """The weights the golden script built: one seed, then every spatial scale in order; the discriminators seeded one by
    one (as tests/test_harness_gpu.py seeds its trainers)."""
    from ir2rgb_amd import networks as N
    seed, ngf = int(g["seed"]), int(g["ngf"])
    tr = trainer(dev, dtype, first_layer_gen_filters=ngf, niter_fix_global=int(g["niter_fix_global"]), lr=float(g["lr"]))
    o = tr.opt
    kw = {k: o[k] for k in ("gen_blocks", "n_local_enhancers", "feat_num", "n_blocks_local", "fg", "no_flow")}
    tG = o["n_input_gen_frames"]
    torch.manual_seed(seed)
    for s in range(2):
        m = N.build_generator_module(o["input_nc"] * tG, o["output_nc"], (tG - 1) * o["output_nc"], ngf // 2 ** s,
                                     o["gen_network"] + ("-local" if s else ""), o["gen_ds_layers"], o["norm"], s, **kw)
        tr.netG[s].load_state_dict(m.state_dict())
    d_in = o["input_nc"] + o["output_nc"]
    torch.manual_seed(seed + 1)
    tr.netD.load_state_dict(N.build_discriminator_module(d_in, o["first_layer_dis_filters"], o["n_layers_D"], o["norm"], o["num_D"],
                                                         not o["no_ganFeat"]).state_dict())
    for s in range(tr.t_scales):
        torch.manual_seed(seed + 2 + s)
        d = N.build_discriminator_module(o["output_nc"] * tr.tD + 2 * (tr.tD - 1), o["first_layer_dis_filters"], o["n_layers_D"],
                                         o["norm"], o["num_D"], not o["no_ganFeat"])
        tr.netD_T[s].load_state_dict(d.state_dict())
    return tr


def rel_l2(a, ref):
    a, ref = a.detach().float().cpu(), torch.from_numpy(np.asarray(ref, dtype=np.float32))
    assert tuple(a.shape) == tuple(ref.shape)
    return ((a - ref).norm() / ref.norm().clamp_min(1e-12)).item()


def _floor_tol(floor, mult=1.5, add=0.02):
    return max(mult * floor, floor + add)


@pytest.mark.parametrize("dtype", DTYPES)
def test_fix_global_windows_vs_reference_golden(dev, golden_dir, dtype):
    """The rule of test_training_windows_vs_reference_golden, restated: window 0 outputs within max(1.5 x floor, floor + 0.02)
    and loss terms within max(3 x floor, 1e-2); window 1 loss terms within max(4 x floor, 2 x SEQ_TOL) (its outputs: as
    there, within the floor rule of their own window); stored gradient tensors within max(2 x floor, floor + 0.03) in relative
    L2, their projection within that or half the L2 floor, the total gradient norm within max(3 x floor, floor + 0.05).  The
    coarse scale's gradient norms are 0 in the golden and its parameters have no gradient here."""
    g = np.load(os.path.join(golden_dir, "window_2scale_fixglobal_ngf64_64x128.npz"))
    fl = "f16" if dtype == torch.float16 else "bf16"
    floor = {k[len(f"floor/{fl}/"):]: float(g[k]) for k in g.files if k.startswith(f"floor/{fl}/")}
    assert int(g["floor_windows"]) == int(g["n_windows"]) == 2
    tr = _seeded(g, dev, dtype)
    assert not tr.finetune_all
    A, B = torch.from_numpy(g["seq_A"].astype(np.float32)).to(dev), torch.from_numpy(g["seq_B"].astype(np.float32)).to(dev)
    tG = tr.opt["n_input_gen_frames"]
    for i in range(2):
        out = tr.train_window(A[:, i:i + tG], B[:, i:i + tG])
        ref = {k.split("/")[-1]: float(g[k]) for k in g.files if k.startswith(f"w{i}/loss/")}
        got = {k: v.item() for k, v in out.items()}
        assert not {k for k in ref if k not in got and not k.startswith("G_T_Warp")} and not set(got) - set(ref)
        errs = {k: abs(got[k] - ref[k]) / max(abs(ref[k]), 0.05) for k in got}
        tols = {k: max(3 * floor[f"w{i}/loss/{k}"], 1e-2) if i == 0 else max(4 * floor[f"w{i}/loss/{k}"], 2 * SEQ_TOL[dtype]) for k in got}
        for name, t in zip(("fake_B", "fake_B_raw", "flow", "weight"), tr.last_outputs):
            errs[name] = rel_l2(t, g[f"w{i}/{name}"].astype(np.float32))
            tols[name] = _floor_tol(floor[f"w{i}/out/{name}"])
        print("fixglobal", dtype, "window", i, {k: (round(v, 4), round(tols[k], 4)) for k, v in errs.items()})
        bad = {k: (v, tols[k]) for k, v in errs.items() if v > tols[k]}
        assert not bad, f"window {i}: (error, tolerance) {bad}"
        if i == 0:
            assert [str(k) for k in g["w0/G0/grad_names"]] == [k for k, _ in tr.netG[0].named_parameters()]
            assert not g["w0/G0/grad_norms"].any() and all(p.grad is None for p in tr.netG[0].parameters())
            for tag, net in (("G1", tr.netG[1]), ("D", tr.netD)):
                params = dict(net.named_parameters())
                assert list(params) == [str(k) for k in g[f"w0/{tag}/grad_names"]]
                tot_h = np.sqrt(sum(float(p.grad.double().pow(2).sum()) for p in params.values() if p.grad is not None))
                tot_r = float(np.sqrt((g[f"w0/{tag}/grad_norms"] ** 2).sum()))
                e = abs(tot_h / tot_r - 1)
                assert e <= _floor_tol(floor[f"{tag}/total_norm"], 3.0, 0.05), (tag, "total gradient norm", e)
                checked = 0
                for key in g.files:
                    if not key.startswith(f"w0/{tag}/grad/"):
                        continue
                    k = key[len(f"w0/{tag}/grad/"):]
                    if f"{tag}/l2/{k}" not in floor:
                        continue      # a bias in front of BatchNorm: zero on both sides
                    a, b = params[k].grad.detach().double().cpu().flatten(), torch.from_numpy(g[key]).double().flatten()
                    l2, pr = ((a - b).norm() / b.norm()).item(), abs((a @ b / (b @ b)).item() - 1.0)
                    print("fixglobal", dtype, tag, k, "l2", round(l2, 4), "floor", round(floor[f"{tag}/l2/{k}"], 4), "proj", round(pr, 4))
                    assert l2 <= _floor_tol(floor[f"{tag}/l2/{k}"], 2.0, 0.03), (tag, k, "relative L2", l2, floor[f"{tag}/l2/{k}"])
                    ptol = max(_floor_tol(floor[f"{tag}/proj/{k}"], 2.0, 0.03), 0.5 * floor[f"{tag}/l2/{k}"])
                    assert pr <= ptol, (tag, k, "projection", pr, floor[f"{tag}/proj/{k}"])
                    checked += 1
                assert checked >= 4, (tag, checked)


# ---------------------------------------------------------------------------------------------
# the learning rate through the kernels
# ---------------------------------------------------------------------------------------------
SHAPES = [(3,), (16, 3, 7, 7), (8193,), (130, 33), (1,)]


def _adam_inputs(dev, steps, scale=1.0):
    g = torch.Generator().manual_seed(23)
    init = [torch.randn(s, generator=g) for s in SHAPES]
    grads = [[(torch.randn(s, generator=g) * scale).to(dev) for s in SHAPES] for _ in range(steps)]
    return init, grads


def _step(opt, params, grads, scaler=None):
    for p, gr in zip(params, grads):
        p.grad = gr.clone()
    if scaler is None:
        opt.step()
    else:
        opt.step(scaler)
        scaler.update([opt])


@pytest.mark.parametrize("scaled", [False, True])
def test_lr_change_between_fused_steps_is_exact(dev, scaled):
    from ir2rgb_amd.optim import FusedAdam, LossScaler
    a, b = 2e-3, 7e-4
    init, grads = _adam_inputs(dev, 4, 8.0 if scaled else 1.0)
    mk = lambda: [torch.nn.Parameter(t.clone().to(dev)) for t in init]  # noqa: E731
    scaler = LossScaler(dev, init_scale=8.0, growth_interval=0) if scaled else None
    p1, p2 = mk(), mk()
    o1 = FusedAdam(p1, lr=a, betas=(0.5, 0.999))
    for i in range(2):
        _step(o1, p1, grads[i], scaler)
    sd = o1.state_dict()
    assert int(sd["state"][0]["step"]) == 2
    with torch.no_grad():
        for q, p in zip(p2, p1):
            q.copy_(p)
    o1.param_groups[0]["lr"] = b
    for i in (2, 3):
        _step(o1, p1, grads[i], scaler)
    o2 = FusedAdam(p2, lr=b, betas=(0.5, 0.999))
    o2.load_state_dict(sd)
    assert o2.lr == a               # (torch.optim's rule: a state_dict carries its rate)
    o2.lr = b
    for i in (2, 3):
        _step(o2, p2, grads[i], scaler)
    assert all(same(x, y) for x, y in zip(p1, p2))
    assert same(o1.exp_avg, o2.exp_avg) and same(o1.exp_avg_sq, o2.exp_avg_sq)
    if scaled:
        assert scaler.stats()["skipped"] == 0
    # and it is not the step at the old rate
    p3 = mk()
    o3 = FusedAdam(p3, lr=a, betas=(0.5, 0.999))
    for i in range(4):
        _step(o3, p3, grads[i], scaler)
    assert not all(same(x, y) for x, y in zip(p1, p3))


@pytest.mark.parametrize("scaled", [False, True])
def test_lr_zero_moves_no_parameter(dev, scaled):
    from ir2rgb_amd.optim import FusedAdam, LossScaler
    init, grads = _adam_inputs(dev, 2)
    ps = [torch.nn.Parameter(t.clone().to(dev)) for t in init]
    scaler = LossScaler(dev, init_scale=4.0, growth_interval=0) if scaled else None
    o = FusedAdam(ps, lr=0.0, betas=(0.5, 0.999))
    m_prev = o.exp_avg.clone()
    for i in range(2):
        _step(o, ps, grads[i], scaler)
        assert all(same(p, t.to(dev)) for p, t in zip(ps, init))
        assert not same(o.exp_avg, m_prev) and o.exp_avg_sq.any()
        m_prev = o.exp_avg.clone()
    o._read_step_count()
    assert o.step_count == 2


def test_lr_changes_against_torch_adam(dev):
    """The same lr changes (the schedule's shape: constant, decayed, zero) on FusedAdam and torch.optim.Adam, under the bound
    of test_fused_adam_matches_torch_adam."""
    from ir2rgb_amd.optim import FusedAdam
    init, grads = _adam_inputs(dev, 6)
    mine = [torch.nn.Parameter(t.clone().to(dev)) for t in init]
    ref = [torch.nn.Parameter(t.clone().to(dev)) for t in init]
    om, orf = FusedAdam(mine, lr=2e-3, betas=(0.5, 0.999)), torch.optim.Adam(ref, lr=2e-3, betas=(0.5, 0.999))
    for i, lr in enumerate((2e-3, 2e-3, 1.8e-3, 1e-3, 2e-4, 0.0)):
        for opt in (om, orf):
            for group in opt.param_groups:
                group["lr"] = lr
        for p, q, gr in zip(mine, ref, grads[i]):
            p.grad, q.grad = gr.clone(), gr.clone()
        om.step(), orf.step()
        for k, (p, q) in enumerate(zip(mine, ref)):
            assert torch.allclose(p, q, rtol=2e-6, atol=1e-7), (i, k, (p - q).abs().max().item())


@pytest.mark.parametrize("fused_adam", [True, False])
@pytest.mark.parametrize("ttur", [False, True])
@pytest.mark.parametrize("policy", ["reference", "all"])
def test_update_learning_rate_policies(dev, policy, ttur, fused_adam):
    from ir2rgb_amd.schedule import TrainingSchedule
    tr = trainer(dev, torch.bfloat16, TTUR=ttur, lr_policy=policy, fused_adam=fused_adam, niter_fix_global=1)
    lr = 2e-4
    rate = lambda o: o.param_groups[0]["lr"]  # noqa: E731
    beta = lambda o: tuple(o.param_groups[0]["betas"])  # noqa: E731
    fg, fd = (0.5, 2.0) if ttur else (1.0, 1.0)
    assert rate(tr.optimizer_G) == lr * fg and rate(tr.optimizer_D) == lr * fd and all(rate(o) == lr for o in tr.optimizer_D_T)
    assert beta(tr.optimizer_G) == beta(tr.optimizer_D) == ((0.0, 0.9) if ttur else (0.5, 0.999))
    assert all(beta(o) == (0.5, 0.999) for o in tr.optimizer_D_T)
    s = TrainingSchedule(niter=10, niter_decay=10, lr=lr, n_scales_spatial=2, niter_fix_global=1)
    tr.attach_schedule(s)
    with pytest.raises(ValueError):
        tr.attach_schedule(TrainingSchedule(lr=1e-3))
    new = tr.update_learning_rate(15)
    assert new == lr * (1 - (15 - 10) / 10) == s.lr_after(15) == tr.old_lr
    if policy == "reference":       # one value on G and D (TTUR's factors are gone), the temporal ones untouched
        assert rate(tr.optimizer_G) == new and rate(tr.optimizer_D) == new and all(rate(o) == lr for o in tr.optimizer_D_T)
    else:
        assert rate(tr.optimizer_G) == new * fg and rate(tr.optimizer_D) == new * fd and all(rate(o) == new for o in tr.optimizer_D_T)
    tr.update_fixed_params()
    keep = policy == "all"
    assert rate(tr.optimizer_G) == new * (fg if keep else 1.0)
    assert beta(tr.optimizer_G) == ((0.0, 0.9) if ttur and keep else (0.5, 0.999))
    assert len(tr.optimizer_G.param_groups[0]["params"]) == sum(1 for g in tr.netG for _ in g.parameters())
    tr.update_learning_rate(20)
    assert rate(tr.optimizer_G) == 0.0 and rate(tr.optimizer_D) == 0.0
    # update_training_batch: the schedule's arithmetic, applied to the trainer
    s4 = TrainingSchedule(lr=lr, max_frames_per_gpu=4, max_frames_backpropagate=4, n_scales_spatial=2, niter_fix_global=1)
    tr.attach_schedule(s4)
    assert tr.update_training_batch(1) == 4 and tr.opt["n_frames_bp"] == 2
    assert tr.update_training_batch(2) == 4 and tr.opt["n_frames_bp"] == 4
    assert tr.update_training_batch(1, resume=True) == 4 and tr.opt["n_frames_bp"] == 2


# ---------------------------------------------------------------------------------------------
# the device loss log
# ---------------------------------------------------------------------------------------------
GUARD = 4096


def _guarded_log(dev, names, capacity):
    """A LossLog whose ring and state live inside canary bands (in the manner of tests/test_bounds_gpu.py)."""
    from ir2rgb_amd.losslog import ABSENT, LossLog
    log = LossLog(dev, names, capacity)
    ring = torch.full((GUARD + log.ring.numel() + GUARD,), 7.0, dtype=torch.float32, device=dev)
    state = torch.full((GUARD + log.state.numel() + GUARD,), 0x0707070707070707, dtype=torch.int64, device=dev)
    log.ring = ring[GUARD:GUARD + log.ring.numel()].view(capacity, 32)
    log.ring.fill_(ABSENT)
    log.state = state[GUARD:GUARD + log.state.numel()]
    log.state.zero_()

    def intact():
        return bool((ring[:GUARD] == 7.0).all() and (ring[-GUARD:] == 7.0).all() and
                    (state[:GUARD] == 0x0707070707070707).all() and (state[-GUARD:] == 0x0707070707070707).all())
    return log, intact


@pytest.mark.parametrize("n", [1, 5, 32])
def test_loss_log_pushes(dev, n):
    from ir2rgb_amd.losslog import ABSENT
    names = [f"t{i}" for i in range(n)]
    log, intact = _guarded_log(dev, names, 4)
    g = torch.Generator().manual_seed(n)
    rows = torch.randn(7, n, generator=g) * 3
    rows[0:3, 0] = torch.tensor([1e8, 1.0, -1e8])              # an fp32 running sum would lose the 1
    absent = {(w, n - 1) for w in (1, 2, 5)} if n > 1 else set()      # the last slot is missing from three windows
    on_dev = rows.to(dev)

    def push(w):
        log.push({names[i]: on_dev[w, i] for i in range(n) if (w, i) not in absent})

    def mean(ws, i):
        vals = [float(rows[w, i]) for w in ws if (w, i) not in absent]
        total = 0.0
        for v in vals:              # left to right, in double: what the kernel does
            total += v
        return total / len(vals) if vals else None

    for w in range(3):
        push(w)
    r = log.read()
    assert r["count"] == 3 and r["skipped"] == 0
    assert r["mean"]["t0"] == mean(range(3), 0) == 1.0 / 3.0
    for i in range(n):
        m = mean(range(3), i)
        assert r["mean"].get(names[i]) == m, (i, r["mean"].get(names[i]), m)
        last = None if (2, i) in absent else float(rows[2, i])
        assert r["last"].get(names[i]) == last
    for w in range(3, 7):
        push(w)
    r = log.read()                  # the sums were reset, the ring was not
    assert r["count"] == 7 and all(r["mean"].get(names[i]) == mean(range(3, 7), i) for i in range(n))
    assert log.read()["mean"] == {} and log.read()["count"] == 7
    ring = log.ring.cpu()
    for w in range(3, 7):           # capacity 4: windows 3..6 are in rows 3, 0, 1, 2
        want = torch.full((32,), ABSENT)
        for i in range(n):
            if (w, i) not in absent:
                want[i] = rows[w, i]
        assert same(ring[w % 4], want), w
    for i in range(n):
        want = torch.tensor([ABSENT if (w, i) in absent else float(rows[w, i]) for w in range(3, 7)])
        assert same(log.history(names[i]), want)
    assert intact()


def test_loss_log_history_before_wrap_and_passthrough(dev):
    """inf and NaN losses are recorded as they are, in the ring and in the mean: the log hides nothing."""
    log, intact = _guarded_log(dev, ["a", "b", "c"], 8)
    vals = torch.tensor([[1.5, float("inf"), 2.0], [2.5, 1.0, float("nan")], [-0.0, -float("inf"), 3.0]], device=dev)
    for w in range(3):
        log.push({"a": vals[w, 0], "b": vals[w, 1], "c": vals[w, 2], "not_logged": vals[w, 0]})
    assert same(log.history("a"), vals[:, 0].cpu()) and same(log.history("b"), vals[:, 1].cpu()) and same(log.history("c"), vals[:, 2].cpu())
    r = log.read()
    assert r["mean"]["a"] == 4.0 / 3.0 and np.isnan(r["mean"]["b"]) and np.isnan(r["mean"]["c"]) and r["skipped"] == 0
    assert r["last"]["b"] == -float("inf") and r["last"]["c"] == 3.0
    log.push({"a": vals[0, 0], "b": vals[0, 1], "c": vals[0, 2]})
    r = log.read()
    assert r["mean"]["b"] == float("inf") and r["mean"]["c"] == 2.0
    with pytest.raises(ValueError):
        log.push({"a": vals[0]})                     # not zero-dimensional
    with pytest.raises(ValueError):
        log.push({"a": vals[0, 0].double()})
    assert intact()


def test_loss_log_skipped_windows(dev):
    from ir2rgb_amd.optim import FusedAdam, LossScaler
    log, intact = _guarded_log(dev, ["a", "b"], 4)
    ps = [[torch.nn.Parameter(torch.ones(5, device=dev))] for _ in range(2)]
    opts = [FusedAdam(p, lr=1e-3) for p in ps]
    scaler = LossScaler(dev, init_scale=4.0, growth_interval=0)
    for o, p in zip(opts, ps):
        p[0].grad = torch.ones(5, device=dev)
        o.step(scaler)
    scaler.update(opts)
    assert scaler.last_optimizers() == opts
    vals = torch.tensor([[1.0, 10.0], [2.0, 20.0], [4.0, 40.0]], device=dev)
    log.push({"a": vals[0, 0], "b": vals[0, 1]}, scaler)                 # a clean window
    opts[1].scaled_state().view(torch.float32)[8] = 1.0                   # found_inf of ir2rgb_adam_state (offset 32)
    log.push({"a": vals[1, 0], "b": vals[1, 1]}, scaler)                 # skipped: in the ring, not in the sums
    opts[1].scaled_state().view(torch.float32)[8] = 0.0
    log.push({"a": vals[2, 0]}, scaler)
    r = log.read()
    assert r["count"] == 3 and r["skipped"] == 1
    assert r["mean"] == {"a": 2.5, "b": 10.0} and r["last"] == {"a": 4.0}
    assert log.history("a").tolist() == [1.0, 2.0, 4.0] and log.history("b").tolist()[:2] == [10.0, 20.0]
    assert log.read()["skipped"] == 0
    assert intact()


def test_loss_log_push_does_not_synchronise(dev, sequence):
    from ir2rgb_amd.losslog import LossLog
    from ir2rgb_amd.training import loss_names
    A, B = sequence
    tr = trainer(dev, torch.float16, loss_scale=256.0)
    log = LossLog(dev, loss_names(tr.t_scales))
    outs = []
    for i in range(3):
        out = tr.train_window(A[:, i:i + 3], B[:, i:i + 3])
        assert set(out) <= set(log.names)
        torch.cuda.set_sync_debug_mode("error")
        try:
            log.push(out, tr.loss_scaler)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        outs.append({k: v.clone() for k, v in out.items()})
    r = log.read()
    assert r["count"] == 3 and r["skipped"] == tr.loss_scaler.stats()["skipped"]
    for k in ("G", "D", "G_GAN", "F_Flow"):
        assert log.history(k).tolist() == [o[k].item() for o in outs]
    assert r["last"]["G"] == outs[-1]["G"].item() and "D_T1" not in r["last"]      # temporal scale 1 needs 7 frames


# ---------------------------------------------------------------------------------------------
# fit
# ---------------------------------------------------------------------------------------------
class _Sequences:
    """Two synthetic sequences of six frames; records what is asked of it and the trainer's state at that moment."""
    seq_len_max = 6

    def __init__(self, dev, trainer_):
        from ir2rgb_amd import vid2vid as V
        self.data = [V.synthetic_sequence(6, 64, 128, 10 + i, dev) for i in range(2)]
        self.tr, self.calls = trainer_, []

    def __len__(self):
        return len(self.data)

    def sequence(self, index, n_frames_total):
        tr = self.tr
        rate = lambda o: o.param_groups[0]["lr"]  # noqa: E731
        self.calls.append(dict(index=index, n=n_frames_total, finetune_all=tr.finetune_all, bp=tr.opt["n_frames_bp"],
                               lr=[rate(tr.optimizer_G), rate(tr.optimizer_D)] + [rate(o) for o in tr.optimizer_D_T],
                               coarse=torch.cat([p.detach().flatten() for p in tr.netG[0].parameters()]).clone()))
        A, B = self.data[index]
        t = n_frames_total + tr.opt["n_input_gen_frames"] - 1
        return A[:, :t], B[:, :t]


def test_fit_end_to_end(dev, tmp_path):
    from test_schedule_cpu import reference_loop
    from ir2rgb_amd import checkpoint, fit
    from ir2rgb_amd.losslog import LossLog
    from ir2rgb_amd.schedule import TrainingSchedule
    from ir2rgb_amd.training import loss_names
    kw = dict(niter=1, niter_decay=2, niter_step=1, niter_fix_global=1, print_freq=2, save_latest_freq=3, n_frames_total=2,
              n_scales_spatial=2, seq_len_max=6)
    s = TrainingSchedule(**kw)
    tr = trainer(dev, torch.bfloat16, niter_fix_global=1)
    seqs = _Sequences(dev, tr)
    log = LossLog(dev, loss_names(tr.t_scales))
    events, lines = [], []
    save_dir = str(tmp_path)
    left = fit(tr, seqs, s, save_dir=save_dir, log=lines.append, loss_log=log, events=events)
    want, want_left = reference_loop(2, 1, 2, 2, 3, 1)
    assert events == want and left == want_left == (4, 0, 6)
    assert checkpoint.read_iter(save_dir) == (4, 0)
    for label in ("latest", "1", "2", "3"):
        for net in ("G0", "G1", "D", "D_T0", "D_T1"):
            assert os.path.isfile(checkpoint.network_path(save_dir, net, label)), (label, net)
    # epochs 1, 2, 3: two sequences each; the sequence length doubles after epoch 1 to the cap 6 - (tG - 1) = 4
    c = seqs.calls
    assert [x["index"] for x in c] == [0, 1] * 3 and [x["n"] for x in c] == [2, 2, 4, 4, 4, 4]
    assert [x["finetune_all"] for x in c] == [False, False, True, True, True, True]
    lr = 2e-4
    assert [x["lr"] for x in c[:4]] == [[lr] * 4] * 4                   # epoch 2 > niter: decayed at its END
    assert [x["lr"] for x in c[4:]] == [[lr * (1 - 1 / 2)] * 2 + [lr] * 2] * 2     # lr_policy="reference": G and D only
    assert tr.optimizer_G.param_groups[0]["lr"] == 0.0 == tr.optimizer_D.param_groups[0]["lr"]
    assert same(c[0]["coarse"], c[1]["coarse"]) and same(c[0]["coarse"], c[2]["coarse"])       # fixed through epoch 1
    assert not same(c[2]["coarse"], c[3]["coarse"]) and not same(c[3]["coarse"], c[4]["coarse"])
    windows = 2 * (2 + 4 + 4)
    assert log.read()["count"] == windows and len(log.history("G")) == windows == len(log.history("D"))
    assert torch.isfinite(log.history("G")).all()
    prints = [ln for ln in lines if ln.startswith("(epoch: ")]
    assert len(prints) == 3 and prints[0].startswith("(epoch: 1, iters: 2, time: ") and " G_GAN: " in prints[0]
    assert any("Now finetuning all scales" in ln for ln in lines) and any(ln.startswith("update learning rate: ") for ln in lines)

    # resume: as if the run had stopped after the save at total_steps 3, which wrote "2,1" (models.py:102)
    assert ("save_latest", 2, 3, (2, 1)) in events
    checkpoint.write_iter(save_dir, 2, 1)
    tr2 = trainer(dev, torch.bfloat16, niter_fix_global=1, seed=5)
    seqs2 = _Sequences(dev, tr2)
    events2 = []
    left2 = fit(tr2, seqs2, s, save_dir=save_dir, log=lines.append, continue_train=True, events=events2)
    want2, want_left2 = reference_loop(2, 1, 2, 2, 3, 1, start_epoch=2, epoch_iter=1)
    assert events2 == want2 and left2 == want_left2
    c2 = seqs2.calls
    assert [x["n"] for x in c2] == [4, 4, 4] and all(x["finetune_all"] for x in c2)      # one sequence left in epoch 2
    assert c2[0]["lr"] == [lr] * 4 and c2[1]["lr"] == [lr / 2, lr / 2, lr, lr]
    assert same(c2[0]["coarse"], torch.cat([p.detach().flatten() for p in tr.netG[0].parameters()]))      # the saved weights
    assert any(ln == "Resuming from epoch 2 at iteration 1" for ln in lines)
