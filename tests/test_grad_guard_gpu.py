"""Guarded optimizer steps on the device (csrc/adam.hip, ir2rgb_amd.optim.GradGuard, the trainer's ``max_grad_norm``).

Kernel level: ``FusedAdam`` over hand-made parameter lists.  The list below puts every size at which the check and the
step take another path on the 16-byte path (its moments start at a multiple of four elements) and fills the gaps with
1- and 3-element tensors, which -- their moments off 16 bytes -- take the element-wise path, as does the tensor whose
parameter storage is offset by 4 bytes.  Everything is compared bit for bit: with max_norm = inf against ir2rgb_adam_step
on the unscaled gradient, with a threshold against ir2rgb_adam_step on the gradient pre-multiplied by the device's
factor, the decision itself with ``decision_errors`` of tests/test_grad_guard_cpu.py (which shows there that it rejects
five faulty rules).  Trainer level: training is bit-reproducible, so the guarded trainer is compared bit for bit too.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_grad_guard_cpu import decision_errors, f32_bits  # noqa: E402
from test_loss_scale_gpu import CANARY, GUARD, _Banded  # noqa: E402
from window_stub import stub_flow_and_conf  # noqa: E402

from ir2rgb_amd import _lib  # noqa: E402
from ir2rgb_amd import optim as OP  # noqa: E402
from ir2rgb_amd.losslog import LossLog  # noqa: E402
from ir2rgb_amd.training import loss_names  # noqa: E402

F = np.float32
INF = float("inf")
LR, B1, B2 = 2e-4, 0.5, 0.999
E = 8192
# (n, parameter storage 16-byte aligned).  Moments live in one flat buffer, so a tensor's moments are 16-byte aligned when
# the elements before it are a multiple of 4: the fillers (1, 3) bring the count back to one before every size under test
MIXED = [(8192, True), (3 * 8192, True), (4, True), (4097, True), (3, True), (8193, True), (3, True), (2 * 8192 + 7, True),
         (1, True), (5, True), (3, True), (8191, True), (1, True), (1, True), (3, True), (3, True), (1, True), (4097, False)]
ON_VEC_PATH = {0: 8192, 1: 3 * 8192, 2: 4, 3: 4097, 5: 8193, 7: 2 * 8192 + 7, 9: 5, 11: 8191, 13: 1, 15: 3}
TABLES = {"mixed": MIXED, "single": [(1, True)]}
I_TAIL, I_ONE, I_OFF = 7, 13, 17            # an n % 4 tail on the 16-byte path, the 1-element tensor on it, the offset tensor


def _values(n, gen, scale):
    """O(1) values with a few at 2^+-20."""
    t = torch.randn(n, generator=gen) * scale
    for k, e in ((n // 3, 20.0), (n // 2, -20.0)):
        if n > 4:
            t[k] = math.copysign(2.0 ** e, float(t[k])) * scale
    return t


class _Params:
    """Parameters and gradients as views into pools with canaries on both sides, and a FusedAdam over them."""

    def __init__(self, dev, specs, seed):
        gen = torch.Generator().manual_seed(seed)
        self.specs, self.dev = specs, dev
        self.p_pools, self.g_pools, self.params = [], [], []
        for n, aligned in specs:
            off = GUARD if aligned else GUARD + 1
            pool = torch.full((n + 2 * GUARD + 4,), CANARY, dtype=torch.float32)
            pool[off:off + n] = _values(n, gen, 0.05)
            pool = pool.to(dev)
            gpool = torch.full((n + 2 * GUARD + 4,), CANARY, dtype=torch.float32, device=dev)
            p = pool[off:off + n].requires_grad_()
            p.grad = gpool[GUARD:GUARD + n]
            assert (p.data_ptr() % 16 == 0) == aligned and p.grad.data_ptr() % 16 == 0
            self.p_pools.append((pool, off))
            self.g_pools.append(gpool)
            self.params.append(p)
        self.opt = OP.FusedAdam(self.params, lr=LR, betas=(B1, B2))
        if specs is MIXED:          # the sizes under test really are on the 16-byte path, the rest is not
            vec = {i for i in range(len(specs)) if all(q % 16 == 0 for q in (self.params[i].data_ptr(), self.opt.moments(i)[0].data_ptr(),
                                                                                self.opt.moments(i)[1].data_ptr()))}
            assert vec == set(ON_VEC_PATH) and all(specs[i][0] == n for i, n in ON_VEC_PATH.items())

    def set_grads(self, host):
        for p, g in zip(self.params, host):
            p.grad.copy_(g)

    def state(self):
        """(every parameter, exp_avg, exp_avg_sq) on the host; asserts the canaries of the parameter and gradient pools."""
        ps = []
        for (n, _), (pool, off), gpool in zip(self.specs, self.p_pools, self.g_pools):
            h, g = pool.detach().cpu(), gpool.cpu()
            assert torch.all(torch.cat([h[:off], h[off + n:]]) == CANARY), f"n={n}: a parameter pool guard was overwritten"
            assert torch.all(torch.cat([g[:GUARD], g[GUARD + n:]]) == CANARY), f"n={n}: a gradient pool guard was overwritten"
            ps.append(h[off:off + n])
        return torch.cat(ps), self.opt.exp_avg.cpu(), self.opt.exp_avg_sq.cpu()


def _host_grads(specs, seed, scale=1.0):
    gen = torch.Generator().manual_seed(seed)
    return [_values(n, gen, 1.0) * scale for n, _ in specs]


def _assert_same_bits(a, b, what):
    for name, x, y in zip(("p", "exp_avg", "exp_avg_sq"), a, b):
        bad = x.view(torch.int32) != y.view(torch.int32)
        assert not bool(bad.any()), f"{what}: {name} differs in {int(bad.sum())} elements, first at {int(bad.nonzero()[0])}"


def _adam_state(opt):
    return _lib.AdamState.from_buffer_copy(opt.scaled_state().cpu().numpy().tobytes())


def _guard_state(guard):
    return _lib.GradGuardState.from_buffer_copy(guard.state.cpu().numpy().tobytes())


def _guarded_step(ps, guard, scaler, inv):
    """One guarded step -> the decision in decision_errors' form (sumsq: the device's own, of the stored gradient)."""
    a0, g0 = _adam_state(ps.opt), _guard_state(guard)
    ps.opt.step(scaler, guard)
    a1, g1 = _adam_state(ps.opt), _guard_state(guard)
    assert ps.opt.last_step_scaled
    return {"found": a1.found_inf != 0.0, "sumsq": a1.grad_sumsq / (inv * inv), "norm": F(g1.grad_norm), "c": F(g1.clip_coef),
            "factor": F(g1.factor), "d_step": a1.step - a0.step, "d_steps": g1.steps - g0.steps,
            "d_clipped": g1.clipped - g0.clipped, "d_skipped": g1.skipped - g0.skipped}


# ---------------------------------------------------------------------------------------------------------------------
# T1: max_norm = inf is the unguarded step, bit for bit
@pytest.mark.parametrize("scale", [None, 2.0 ** 12])
@pytest.mark.parametrize("table", list(TABLES))
def test_infinite_threshold_is_the_unguarded_step(dev, table, scale):
    """The reference is the plain step (ir2rgb_adam_step, the host's coefficients) on the gradient times 1 / scale, a
    product that is exact for the power of two here.  With a scale, a third optimizer takes the step with the scaler alone
    (no guard block): its ir2rgb_adam_state must be the guarded one's byte for byte."""
    specs = TABLES[table]
    inv = 1.0 / (scale or 1.0)
    a, b = _Params(dev, specs, 1), _Params(dev, specs, 1)
    guard = OP.GradGuard(a.opt, INF)
    sa = c = sc = None
    if scale is not None:
        sa, sc = OP.LossScaler(dev, init_scale=scale, growth_interval=0), OP.LossScaler(dev, init_scale=scale, growth_interval=0)
        c = _Params(dev, specs, 1)
    for step in range(3):
        host = _host_grads(specs, 10 + step, scale or 1.0)
        unscaled = [torch.from_numpy(g.numpy() * F(inv)) for g in host]
        assert all(torch.equal(u.double(), g.double() * inv) for u, g in zip(unscaled, host))      # exact
        a.set_grads(host), b.set_grads(unscaled)
        got = _guarded_step(a, guard, sa, inv)
        b.opt.step()               # ir2rgb_adam_step
        assert not b.opt.last_step_scaled
        assert decision_errors(got, host, INF, inv) == []
        assert float(got["c"]) == 1.0 and float(got["factor"]) == inv
        assert f32_bits(_adam_state(a.opt).factor) == f32_bits(inv)
        _assert_same_bits(a.state(), b.state(), f"{table} scale {scale} step {step + 1}")
        if c is not None:          # scaler only (guard_state NULL) against scaler + guard at inf
            c.set_grads(host)
            c.opt.step(sc)
            assert bytes(_adam_state(a.opt)) == bytes(_adam_state(c.opt))
    assert _guard_state(guard).steps == 3 and _guard_state(guard).clipped == 0 and _adam_state(a.opt).step == 3


# ---------------------------------------------------------------------------------------------------------------------
# T2: clipping
@pytest.mark.parametrize("scale", [None, 2.0 ** 12])
@pytest.mark.parametrize("table", list(TABLES))
def test_clipped_step_is_the_plain_step_on_the_multiplied_gradient(dev, table, scale):
    specs = TABLES[table]
    inv = 1.0 / (scale or 1.0)
    a, b = _Params(dev, specs, 2), _Params(dev, specs, 2)
    scaler = None if scale is None else OP.LossScaler(dev, init_scale=scale, growth_interval=0)
    for step in range(2):
        host = _host_grads(specs, 20 + step, scale or 1.0)
        max_norm = float(F(0.3 * OP.grad_guard_reference(host, INF, inv)[2]))       # 0.3 x this step's reference norm
        guard = OP.GradGuard(a.opt, max_norm)
        a.set_grads(host)
        got = _guarded_step(a, guard, scaler, inv)
        print(table, scale, "step", step + 1, {k: (float(v) if not isinstance(v, (bool, int)) else v) for k, v in got.items()},
              "reference", OP.grad_guard_reference(host, max_norm, inv))
        assert decision_errors(got, host, max_norm, inv) == []
        assert float(got["c"]) < 1.0 and got["d_clipped"] == 1
        b.set_grads([torch.from_numpy(g.numpy() * got["factor"]) for g in host])      # one rounded fp32 product per element
        b.opt.step()
        _assert_same_bits(a.state(), b.state(), f"{table} scale {scale} step {step + 1}")
    assert guard.stats() == {"steps": 1, "clipped": 1, "skipped": 0, "grad_norm": float(got["norm"]), "clip_coef": float(got["c"])}
    assert guard.norm_tensor.dim() == 0 and guard.norm_tensor.dtype == torch.float32 and guard.norm_tensor.item() == float(got["norm"])


# ---------------------------------------------------------------------------------------------------------------------
# T3: both sides of the threshold
def test_both_sides_of_the_threshold(dev):
    ps = _Params(dev, MIXED, 3)
    host = [torch.zeros(n) for n, _ in MIXED]
    host[I_TAIL][-1] = host[I_ONE][0] = host[I_OFF][100] = host[0][0] = 0.5           # norm exactly 1
    edge = 1.0 + 1e-6                                                              # norm + 1e-6 as the rule forms it
    below = F(edge) if float(F(edge)) < edge else np.nextafter(F(edge), F(0))
    above = np.nextafter(below, F(2))
    assert float(below) < edge < float(above)
    for x, clipped in ((float(above), 0), (float(below), 1)):
        guard = OP.GradGuard(ps.opt, x)
        ps.set_grads(host)
        got = _guarded_step(ps, guard, None, 1.0)
        assert float(got["norm"]) == 1.0 and got["sumsq"] == 1.0
        assert decision_errors(got, host, x) == []
        assert guard.stats()["clipped"] == clipped == int(float(got["c"]) < 1.0)


# ---------------------------------------------------------------------------------------------------------------------
# T4: a non-finite gradient skips the step
PLANTS = {"first": (0, 0), "last": (len(MIXED) - 1, 4096), "tail": (I_TAIL, 2 * 8192 + 6), "one_element": (I_ONE, 0),
          "misaligned": (I_OFF, 2000)}


@pytest.mark.parametrize("special", [INF, -INF, math.nan], ids=["inf", "neginf", "nan"])
@pytest.mark.parametrize("where", list(PLANTS) + ["single"])
def test_non_finite_gradient_skips_the_step(dev, where, special):
    specs = TABLES["single"] if where == "single" else MIXED
    i, e = (0, 0) if where == "single" else PLANTS[where]
    ps = _Params(dev, specs, 4)
    guard = OP.GradGuard(ps.opt, 1.0)
    ema = OP.ParamEMA(ps.params, 0.999)
    ps.set_grads(_host_grads(specs, 40))
    assert decision_errors(_guarded_step(ps, guard, None, 1.0), _host_grads(specs, 40), 1.0) == []
    ema.update(ps.opt)
    before, shadow, coef = ps.state(), ema.buf.clone(), bytes(_adam_state(ps.opt))[:32]
    host = _host_grads(specs, 41)
    host[i][e] = special
    ps.set_grads(host)
    got = _guarded_step(ps, guard, None, 1.0)
    assert got["found"] and decision_errors(got, host, 1.0) == []
    _assert_same_bits(ps.state(), before, f"{where}: a skipped step")
    st = _adam_state(ps.opt)
    assert st.step == 1 and st.found_inf == 1.0 and bytes(st)[:32] == coef
    assert guard.stats()["skipped"] == 1 and guard.stats()["steps"] == 1 and not math.isfinite(guard.stats()["grad_norm"])
    ema.update(ps.opt)
    assert torch.equal(shadow.view(torch.int32), ema.buf.view(torch.int32)), "the average moved after a skipped step"
    assert (ema.stats()["updates"], ema.stats()["skipped"]) == (1, 1)
    # the next finite step is step 2
    host = _host_grads(specs, 42)
    ps.set_grads(host)
    got = _guarded_step(ps, guard, None, 1.0)
    assert decision_errors(got, host, 1.0) == [] and _adam_state(ps.opt).step == 2
    after = ps.state()
    assert not torch.equal(after[0], before[0]) and bool(torch.isfinite(torch.cat(after)).all())
    ema.update(ps.opt)
    assert (ema.stats()["updates"], ema.stats()["skipped"]) == (2, 1)
    assert ps.opt.state_dict()["state"][0]["step"].item() == 2.0


# ---------------------------------------------------------------------------------------------------------------------
# T5: the entry points' refusals
def test_entry_points_refuse_bad_arguments(dev):
    assert _lib.query("ir2rgb_grad_guard_state_bytes") == 32
    ps = _Params(dev, TABLES["single"], 5)
    ps.set_grads(_host_grads(TABLES["single"], 50))
    ps.opt._refresh_table()
    before = ps.state()
    st = _Banded(dev, _lib.query("ir2rgb_loss_scale_state_bytes", 0), _lib.AdamState(step=4))
    gs = _Banded(dev, 32, _lib.GradGuardState(steps=4, clipped=1, skipped=2))
    sc = _Banded(dev, _lib.query("ir2rgb_loss_scale_state_bytes", 1), _lib.LossScaleState(scale=4.0, inv_scale=0.25))
    part = _Banded(dev, _lib.query("ir2rgb_grad_check_partial_bytes", 1))
    lib, stream = _lib.lib(), _lib.current_stream(ps.opt.exp_avg)
    tab, blk = ps.opt._rows_dev, ps.opt._blocks
    good = (tab, blk, 1, part.ptr, st.ptr, gs.ptr, sc.ptr, 1.0, LR, B1, B2, 1e-8)

    def check(**kw):
        names = ("table", "blocks", "nblocks", "partial", "opt_state", "guard_state", "scaler_state", "max_norm", "lr", "beta1",
                 "beta2", "eps")
        return lib.ir2rgb_grad_check(*[kw.get(n, v) for n, v in zip(names, good)], stream)

    for kw in (dict(table=None), dict(blocks=None), dict(partial=None), dict(opt_state=None), dict(nblocks=-1),
               dict(max_norm=0.0), dict(max_norm=-1.0), dict(max_norm=math.nan), dict(max_norm=-INF), dict(beta1=1.0), dict(beta2=-0.1)):
        assert check(**kw) == -1, kw
    for kw in (dict(partial=part.ptr + 4), dict(opt_state=st.ptr + 4), dict(guard_state=gs.ptr + 2), dict(scaler_state=sc.ptr + 2)):
        assert check(**kw) == -3, kw
    step_good = (tab, blk, 1, st.ptr)
    for i in (0, 1, 3):
        assert lib.ir2rgb_adam_step_checked(*[None if j == i else v for j, v in enumerate(step_good)], stream) == -1
    assert lib.ir2rgb_adam_step_checked(tab, blk, -1, st.ptr, stream) == -1
    assert lib.ir2rgb_adam_step_checked(tab, blk, 1, st.ptr + 4, stream) == -3
    assert lib.ir2rgb_adam_step_checked(tab, blk, 0, st.ptr, stream) == 0
    with pytest.raises(ValueError, match="grad_check"):
        _lib.launch("ir2rgb_grad_check", ps.opt.exp_avg, *good[:7], 0.0, *good[8:])
    torch.cuda.synchronize()
    # refused before any launch: nothing was written
    assert st.bytes() == bytes(_lib.AdamState(step=4)) and gs.bytes() == bytes(_lib.GradGuardState(steps=4, clipped=1, skipped=2))
    part.bytes(), sc.bytes()
    _assert_same_bits(ps.state(), before, "refused calls")
    # +inf is a threshold, a NULL scaler is inv_scale 1, and a scaler's inv_scale enters the norm
    g = float(ps.params[0].grad.item())
    assert check(max_norm=INF, scaler_state=None) == 0 and check(max_norm=INF) == 0
    torch.cuda.synchronize()
    got = _lib.GradGuardState.from_buffer_copy(gs.bytes())
    assert (got.steps, got.clipped, got.skipped, got.clip_coef, got.factor) == (6, 1, 2, 1.0, 0.25)
    assert f32_bits(got.grad_norm) == f32_bits(abs(g) * 0.25)
    # a NULL guard block is accepted, and the banded guard block that was not passed keeps its bytes
    kept = gs.bytes()
    assert check(guard_state=None) == 0 and check(guard_state=None, max_norm=INF, scaler_state=None) == 0
    torch.cuda.synchronize()
    assert gs.bytes() == kept
    after = _lib.AdamState.from_buffer_copy(st.bytes())
    assert (after.step, after.found_inf, after.factor) == (8, 0.0, 1.0)
    part.bytes(), sc.bytes()
    with pytest.raises(ValueError, match="another optimizer"):
        ps.opt.step(None, OP.GradGuard(_Params(dev, TABLES["single"], 6).opt, 1.0))


def test_guarded_step_never_synchronises(dev):
    ps = _Params(dev, [(5, True), (8193, True), (100, True)], 7)
    guard = OP.GradGuard(ps.opt, 0.5)
    ema = OP.ParamEMA(ps.params, 0.999)
    log = LossLog(dev, ["GN"])
    ps.set_grads(_host_grads(ps.specs, 70))

    def window():
        ps.opt.step(None, guard)
        ema.update(ps.opt)
        log.push({"GN": guard.norm_tensor}, None, [ps.opt])

    for _ in range(3):
        window()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(3):
            window()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert guard.stats()["steps"] == 6 and ema.stats()["updates"] == 6
    assert log.history("GN").tolist() == [guard.stats()["grad_norm"]] * 6 and log.read()["skipped"] == 0


# ---------------------------------------------------------------------------------------------------------------------
# the trainer
KW = dict(first_layer_gen_filters=32, n_scales_spatial=2)


def _trainer(dev, dtype, **kw):
    from ir2rgb_amd import vid2vid as V
    tr = V.Vid2VidTrainer(dev, compute_dtype=dtype, build_flow_net=False, **dict(KW, **kw))
    tr.flow_net = stub_flow_and_conf
    return tr


def _optimizers(tr):
    return [tr.optimizer_G, tr.optimizer_D] + list(tr.optimizer_D_T)


def _state(tr):
    return [(torch.cat([p.detach().flatten() for p in o.params]).cpu(), o.exp_avg.cpu(), o.exp_avg_sq.cpu()) for o in _optimizers(tr)]


def _windows(dev, n):
    from ir2rgb_amd import vid2vid as V
    A, Bs = V.synthetic_sequence(n + 2, 64, 128, 3, dev)
    return [(A[:, w:w + 3], Bs[:, w:w + 3]) for w in range(n)]


STEP_ENTRIES = {"ir2rgb_adam_step", "ir2rgb_grad_check", "ir2rgb_adam_step_checked"}


def _launch_names(monkeypatch):
    names = []
    inner = _lib.launch

    def launch(name, *a):
        names.append(name)
        return inner(name, *a)

    monkeypatch.setattr(_lib, "launch", launch)
    return names


@pytest.fixture(scope="module")
def bf16_runs(dev):
    """Three windows of the unguarded bf16 trainer and of the one guarded at inf: (losses per window, state, trainer)."""
    runs = {}
    for name, kw in (("plain", {}), ("inf", {"max_grad_norm": INF})):
        tr = _trainer(dev, torch.bfloat16, **kw)
        outs, after0 = [], None
        for w, (a, b) in enumerate(_windows(dev, 3)):
            outs.append({k: v.clone() for k, v in tr.train_window(a, b).items()})
            if w == 0:
                after0 = _state(tr)
        runs[name] = (outs, _state(tr), tr, after0)
    return runs


def _assert_same_run(a, b, what):
    for w, (la, lb) in enumerate(zip(a[0], b[0])):
        assert {k for k in lb if not k.startswith("GN_")} == set(la)
        for k in la:
            assert la[k].item() == lb[k].item(), (what, w, k, la[k].item(), lb[k].item())
    for i, (sa, sb) in enumerate(zip(a[1], b[1])):
        _assert_same_bits(sa, sb, f"{what}: optimizer {i}")


def test_trainer_without_the_option_is_todays(dev, monkeypatch, bf16_runs):
    names = _launch_names(monkeypatch)
    tr = _trainer(dev, torch.bfloat16)
    assert tr.grad_guards is None and tr.decided_optimizers() is None and tr.opt["max_grad_norm"] is None
    with pytest.raises(ValueError, match="max_grad_norm"):
        tr.grad_guard_stats()
    for a, b in _windows(dev, 2):
        out = tr.train_window(a, b)
        assert not any(k.startswith("GN_") for k in out)
    steps = [n for n in names if n in STEP_ENTRIES]
    assert steps and set(steps) == {"ir2rgb_adam_step"}, set(steps)
    assert all(o._state is None and o._partial is None and not o.last_step_scaled for o in _optimizers(tr))
    assert bf16_runs["plain"][2].grad_guards is None


def test_trainer_bf16_guard_at_inf_changes_no_bit(dev, monkeypatch, bf16_runs):
    plain, guarded = bf16_runs["plain"], bf16_runs["inf"]
    _assert_same_run(plain, guarded, "bf16, max_grad_norm=inf")
    tr = guarded[2]
    stats = tr.grad_guard_stats()
    assert stats["G"]["steps"] == stats["D"]["steps"] == 3 and stats["G"]["clipped"] == stats["G"]["skipped"] == 0
    assert all(s["clipped"] == s["skipped"] == 0 for s in [stats["D"]] + stats["D_T"])
    last = guarded[0][-1]
    assert last["GN_G"].item() == stats["G"]["grad_norm"] > 0 and last["GN_D"].item() == stats["D"]["grad_norm"] > 0
    names = _launch_names(monkeypatch)
    a, b = _windows(dev, 4)[3]
    tr.train_window(a, b)
    steps = {n for n in names if n in STEP_ENTRIES}
    assert steps == {"ir2rgb_grad_check", "ir2rgb_adam_step_checked"}, steps
    assert tr.decided_optimizers() == _optimizers(tr)[:len(tr.decided_optimizers())]


def test_trainer_f16_dynamic_scale_guard_at_inf_changes_no_bit(dev):
    runs = []
    for kw in ({}, {"max_grad_norm": INF}):
        tr = _trainer(dev, torch.float16, loss_scale="dynamic", **kw)
        outs = [{k: v.clone() for k, v in tr.train_window(a, b).items()} for a, b in _windows(dev, 3)]
        runs.append((outs, _state(tr), tr))
    _assert_same_run(runs[0], runs[1], "f16 dynamic, max_grad_norm=inf")
    assert runs[0][2].loss_scaler.state_dict() == runs[1][2].loss_scaler.state_dict()
    skipped = runs[0][2].loss_scaler.stats()["skipped"]
    stats = runs[1][2].grad_guard_stats()
    print("windows skipped by the scaler:", skipped, "guard stats:", stats)
    assert stats["G"]["steps"] + stats["G"]["skipped"] == 3 and stats["G"]["clipped"] == 0


def test_trainer_nan_input_skips_the_window_and_training_goes_on(dev):
    """One NaN pixel in the second window's input_A.  Guarded: that window changes nothing and is logged as skipped.  The
    generated-frame recurrence carries the NaN to the end of its sequence, so the clean window that follows starts the
    next sequence (``reset_sequence``).  Unguarded, the same plant leaves NaN parameters: the plant is live."""
    wins = _windows(dev, 3)
    poisoned = wins[1][0].clone()
    poisoned[0, 2, 1, 20, 40] = math.nan
    tr = _trainer(dev, torch.bfloat16, max_grad_norm=INF, ema_decay=0.999)
    log = LossLog(dev, loss_names(2, grad_norms=True))
    log.push(tr.train_window(*wins[0]), tr.loss_scaler, tr.decided_optimizers())
    before, shadow, ema0 = _state(tr), tr.ema.buf.clone(), tr.ema.stats()
    out = tr.train_window(poisoned, wins[1][1])
    log.push(out, tr.loss_scaler, tr.decided_optimizers())
    assert math.isnan(out["G"].item())
    stepped = tr.decided_optimizers()
    assert stepped[:2] == [tr.optimizer_G, tr.optimizer_D]
    for i, (sb, sa) in enumerate(zip(before, _state(tr))):
        _assert_same_bits(sa, sb, f"optimizer {i} after the poisoned window")
    assert torch.equal(shadow.view(torch.int32), tr.ema.buf.view(torch.int32)), "the average moved in the poisoned window"
    assert tr.ema.stats()["skipped"] == ema0["skipped"] + 1 and tr.ema.stats()["updates"] == ema0["updates"]
    stats = tr.grad_guard_stats()
    assert (stats["G"]["steps"], stats["G"]["skipped"]) == (1, 1) and (stats["D"]["steps"], stats["D"]["skipped"]) == (1, 1)
    assert all(int(o.scaled_state()[0].item()) == 1 for o in stepped[:2])       # the step counts stayed
    tr.reset_sequence()
    out = tr.train_window(*wins[2])
    log.push(out, tr.loss_scaler, tr.decided_optimizers())
    assert all(math.isfinite(v.item()) for v in out.values()), {k: v.item() for k, v in out.items()}
    after = _state(tr)
    assert all(bool(torch.isfinite(t).all()) for s in after for t in s) and bool(torch.isfinite(tr.ema.buf).all())
    assert not torch.equal(after[0][0], before[0][0]) and tr.grad_guard_stats()["G"]["steps"] == 2
    hist = log.history("GN_G")
    assert len(hist) == 3 and math.isfinite(hist[0]) and not math.isfinite(hist[1]) and math.isfinite(hist[2])
    r = log.read()
    assert r["count"] == 3 and r["skipped"] == 1
    assert all(math.isfinite(v) for v in r["mean"].values()) and "GN_G" in r["mean"] and "G" in r["mean"]
    assert abs(r["mean"]["GN_G"] - (float(hist[0]) + float(hist[2])) / 2) <= 1e-6 * r["mean"]["GN_G"]
    # the same plant without the option
    plain = _trainer(dev, torch.bfloat16)
    plain.train_window(*wins[0])
    plain.train_window(poisoned, wins[1][1])
    assert any(bool(torch.isnan(s[0]).any()) for s in _state(plain)[:2]), "the plant did not reach the unguarded parameters"


def test_trainer_threshold_on_the_generator_only(dev, bf16_runs):
    inf_run = bf16_runs["inf"]
    gn0 = inf_run[0][0]["GN_G"].item()
    assert math.isfinite(gn0) and gn0 > 0
    x = 0.5 * gn0
    tr = _trainer(dev, torch.bfloat16, max_grad_norm={"G": x})
    assert tr.grad_guards["G"].max_norm == float(F(x)) and tr.grad_guards["D"].max_norm == INF
    log = LossLog(dev, loss_names(2, grad_norms=True))
    for w, (a, b) in enumerate(_windows(dev, 3)[:2]):       # (the fixture's sequence)
        log.push(tr.train_window(a, b), tr.loss_scaler, tr.decided_optimizers())
        if w == 0:
            after0 = _state(tr)
        assert log.history("GN_G")[w].item() == tr.grad_guards["G"].stats()["grad_norm"]
    assert log.history("GN_G")[0].item() == gn0, "window 0's gradient does not depend on the threshold"
    stats = tr.grad_guard_stats()
    assert stats["G"]["clipped"] >= 1 and stats["D"]["clipped"] == 0 and all(s["clipped"] == 0 for s in stats["D_T"])
    assert stats["G"]["clip_coef"] < 1.0 and stats["D"]["clip_coef"] == 1.0
    _assert_same_bits(after0[1], inf_run[3][1], "D after window 0, threshold on G only")
    assert not torch.equal(after0[0][0], inf_run[3][0][0]), "the generator's clipped step equals the unclipped one"


def test_update_fixed_params_rebuilds_the_generator_guard_and_keeps_its_counters(dev):
    tr = _trainer(dev, torch.bfloat16, max_grad_norm={"G": 1e-3}, niter_fix_global=1)
    wins = _windows(dev, 2)
    tr.train_window(*wins[0])
    old = tr.grad_guards["G"]
    assert tr.grad_guard_stats()["G"]["steps"] == 1
    tr.update_fixed_params()
    assert tr.grad_guards["G"] is not old and tr.grad_guards["G"].optimizer is tr.optimizer_G and tr.grad_guards["G"].max_norm == float(F(1e-3))
    tr.train_window(*wins[1])
    stats = tr.grad_guard_stats()
    assert stats["G"]["steps"] == 2 and tr.grad_guards["G"].stats()["steps"] == 1 and stats["G"]["clipped"] == 2
