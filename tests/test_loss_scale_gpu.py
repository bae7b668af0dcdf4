"""Dynamic loss scaling on the device (csrc/adam.hip, csrc/loss_scale.hip, ir2rgb_amd.optim.LossScaler, the trainer's ``loss_scale``).

Kernel level: the gradient check at every path of its three-way split with inf / NaN planted where each path could miss
them; the skipped step; the scaled step against the fp64 Adam reference under the bounds oracle/replay_ops.replay_adam
applies, and -- a power-of-two scale being exact -- bit for bit against ir2rgb_adam_step on the pre-divided gradient.
Trainer level: the backward pass is linear in the upstream gradient and training is bit-reproducible, so a power-of-two
scale is tested with tolerance 0.

Half stores on the gradient path: that an fp32 -> f16 store overflows to inf and never saturates, keeps subnormals, and
that an inf / NaN of a backward pass stays one is tested kernel by kernel in tests/test_range_gpu.py (the EDGE_RANGE
records of oracle/edge_records.py), not here; the f16 test below starts from a scale whose first gradient is already inf.
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
from window_stub import smooth, stub_flow_and_conf  # noqa: E402

from ir2rgb_amd import _lib  # noqa: E402
from ir2rgb_amd import optim as OP  # noqa: E402
from oracle import bounds as B  # noqa: E402
from oracle import window_ops_ref as O  # noqa: E402

LR, B1, B2, EPS = 2e-4, 0.5, 0.999, 1e-8
E = 8192                                  # ir2rgb_adam_chunk_elems(), asserted below
# (n, every array 16-byte aligned): one element, an n % 4 tail alone, one float4, float4 + tail, the chunk boundary from
# both sides, three chunks with a tail; and one tensor at a 4-byte offset (the scalar path), two chunks with a ragged end
SPECS = [(n, True) for n in (1, 3, 4, 5, 8191, 8192, 8193, 2 * 8192 + 7)] + [(8192 + 5, False)]
N_TOTAL = sum(n for n, _ in SPECS)
GUARD = 8
CANARY = 777.0
BAND = 16                                 # int32 words of canary on both sides of a state block / the partial rows
CANARY_I = 0x5A5A5A5A


def _pool(n, aligned, fill, dev):
    off = GUARD if aligned else GUARD + 1
    pool = torch.full((n + 2 * GUARD + 4,), CANARY, dtype=torch.float32)
    pool[off:off + n] = fill
    return pool.to(dev), off


class _Table:
    """The {p, g, m, v, n} table over SPECS, each array in a pool of its own with guard floats on both sides."""

    def __init__(self, dev, host):
        assert _lib.lib().ir2rgb_adam_chunk_elems() == E
        rows, blocks, self.pools = [], [], []
        for i, ((n, aligned), arrs) in enumerate(zip(SPECS, host)):
            pl = [_pool(n, aligned, t, dev) for t in arrs]
            ptrs = [p.data_ptr() + 4 * off for p, off in pl]
            assert all(q % 16 == 0 for q in ptrs) == aligned
            rows.append(ptrs + [n])
            blocks += [(i, c) for c in range(-(-n // E))]
            self.pools.append(pl)
        self.table = torch.tensor(rows, dtype=torch.int64, device=dev)
        self.blocks = torch.tensor(blocks, dtype=torch.int32, device=dev)
        self.nblocks = len(blocks)

    def read(self):
        """-> per tensor [p, g, m, v] on the host; asserts the guards."""
        out = []
        for (n, aligned), pl in zip(SPECS, self.pools):
            got = []
            for pool, off in pl:
                h = pool.cpu()
                assert torch.all(torch.cat([h[:off], h[off + n:]]) == CANARY), f"n={n} aligned={aligned}: a pool guard was overwritten"
                got.append(h[off:off + n].clone())
            out.append(got)
        return out


def _host_arrays(seed, step, gscale=1.0):
    g = torch.Generator().manual_seed(seed)
    host = []
    for n, _ in SPECS:
        p = torch.randn(n, generator=g) * 0.05
        gr = torch.randn(n, generator=g) * 0.01
        m = torch.zeros(n) if step == 1 else torch.randn(n, generator=g) * 0.01
        v = torch.zeros(n) if step == 1 else torch.rand(n, generator=g) * 1e-4
        host.append([p, gr * gscale, m, v])
    return host


class _Banded:
    """A device block of ``nbytes`` between two canary bands."""

    def __init__(self, dev, nbytes, init=None):
        assert nbytes % 4 == 0
        self.words = nbytes // 4
        buf = torch.full((2 * BAND + self.words,), CANARY_I, dtype=torch.int32)
        buf[BAND:BAND + self.words] = 0 if init is None else torch.frombuffer(bytearray(bytes(init)), dtype=torch.int32)
        self.buf = buf.to(dev)
        self.ptr = self.buf.data_ptr() + 4 * BAND
        assert self.ptr % 16 == 0

    def bytes(self):
        h = self.buf.cpu()
        assert torch.all(h[:BAND] == CANARY_I) and torch.all(h[BAND + self.words:] == CANARY_I), "a canary band was overwritten"
        return h[BAND:BAND + self.words].numpy().tobytes()


def _scaler_block(dev, scale):
    scale = float(np.float32(scale))
    return _Banded(dev, _lib.query("ir2rgb_loss_scale_state_bytes", 1),
                   _lib.LossScaleState(scale=scale, inv_scale=float(np.float32(1.0 / scale)), growth_tracker=0, skipped=0))


def _factor_bits(st):
    return int(np.float32(st.factor).view(np.int32))


def _inv_scale_bits(scale):
    """The bits of the inv_scale a scaler block of ``scale`` holds (_scaler_block)."""
    return int(np.float32(1.0 / float(np.float32(scale))).view(np.int32))


def _check(dev, tab, scale, step0):
    """ir2rgb_grad_check (no guard block, max_norm inf) on a fresh state -> (AdamState, raw state bytes, raw partial bytes, scaler block, state block)."""
    st = _Banded(dev, _lib.query("ir2rgb_loss_scale_state_bytes", 0), _lib.AdamState(step=step0))
    sc = _scaler_block(dev, scale)
    part = _Banded(dev, _lib.query("ir2rgb_grad_check_partial_bytes", tab.nblocks))
    _lib.launch("ir2rgb_grad_check", tab.table, tab.table, tab.blocks, tab.nblocks, part.ptr, st.ptr, None, sc.ptr, math.inf, LR, B1, B2, EPS)
    torch.cuda.synchronize()
    raw = st.bytes()
    assert sc.bytes() == bytes(_lib.LossScaleState(scale=scale, inv_scale=float(np.float32(1.0 / scale)))), "the check wrote the scaler state"
    return _lib.AdamState.from_buffer_copy(raw), raw, part.bytes(), sc, st


# ---------------------------------------------------------------------------------------------------------------------
# the check kernels
PLANTS = {
    "nothing": None,
    "inf_last_of_tail": (7, 2 * 8192 + 6, float("inf")),      # the last element of an n % 4 tail
    "nan_first": (0, 0, float("nan")),                        # element 0 of the first tensor
    "neginf_mid_chunk": (6, 4000, float("-inf")),             # the middle of a whole chunk (n = 8193: chunk 0)
    "neginf_scalar_path": (8, 8192 + 4, float("-inf")),       # the last element of the tensor on the scalar path
    "finite_3e38": (5, None, 3e38),                           # everywhere in one tensor: finite, its square is not a float
}


@pytest.mark.parametrize("plant", list(PLANTS))
def test_grad_check_flag_norm_repeatability_and_canaries(dev, plant):
    scale = 256.0
    host = _host_arrays(11, 2, gscale=scale)
    if PLANTS[plant] is not None:
        i, e, val = PLANTS[plant]
        if e is None:
            host[i][1].fill_(val)
        else:
            host[i][1][e] = val
    tab = _Table(dev, host)
    st, raw, praw, _, _ = _check(dev, tab, scale, step0=6)
    st2, raw2, praw2, _, _ = _check(dev, tab, scale, step0=6)
    assert raw == raw2 and praw == praw2, "the check does not repeat bit for bit"
    want_found = plant not in ("nothing", "finite_3e38")
    assert st.found_inf == (1.0 if want_found else 0.0)
    assert st.step == (6 if want_found else 7)                # the step count advances only for a finite gradient
    # the factor the step multiplies by: the scaler block's inv_scale bit for bit, +0.0 after a non-finite gradient
    assert _factor_bits(st) == (0 if want_found else _inv_scale_bits(scale))
    ref = float(sum((arrs[1].double() ** 2).sum() for arrs in host)) * (1.0 / scale) ** 2
    bound = (N_TOTAL + 2) * 2.0 ** -53
    if math.isfinite(ref):
        err = abs(st.grad_sumsq - ref) / ref
        print(plant, "grad_sumsq", st.grad_sumsq, "fp64 reference", ref, "relative error", err, "bound", bound)
        assert err <= bound
    else:
        print(plant, "grad_sumsq", st.grad_sumsq, "fp64 reference", ref)
        assert math.isnan(st.grad_sumsq) == math.isnan(ref) and math.isinf(st.grad_sumsq) == math.isinf(ref)
    found_r, sumsq_r, _ = OP.grad_check_reference([arrs[1] for arrs in host], 1.0 / scale)
    assert found_r.item() == st.found_inf
    if math.isfinite(ref):
        assert abs(sumsq_r.item() - ref) <= bound * ref
    after = tab.read()                                        # guards intact, nothing written
    for arrs, got in zip(host, after):
        for a, b in zip(arrs, got):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    if not want_found:                                        # the coefficients of step 7, as the host evaluates them
        assert _ulps(_device_coef(st), _host_coef(7)).max() <= 1


def _host_coef(step):
    """The AdamCoef ir2rgb_adam_step's host code evaluates (csrc/adam.h adam_coef), restated."""
    f = np.float32
    lr, b1, b2 = float(f(LR)), float(f(B1)), float(f(B2))
    bc1, bc2 = 1.0 - math.pow(b1, step), 1.0 - math.pow(b2, step)
    return np.array([lr / bc1, b1, b2, 1.0 - b1, 1.0 - b2, math.sqrt(bc2), float(f(EPS))]).astype(f)


def _device_coef(st):
    return np.array([st.step_size, st.beta1, st.beta2, st.omb1, st.omb2, st.bc2_sqrt, st.eps], dtype=np.float32)


def _ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


# ---------------------------------------------------------------------------------------------------------------------
# the scaled step
def _scaled_step(dev, host_scaled, scale, step):
    tab = _Table(dev, host_scaled)
    st = _Banded(dev, _lib.query("ir2rgb_loss_scale_state_bytes", 0), _lib.AdamState(step=step - 1))
    sc = _scaler_block(dev, scale)
    part = _Banded(dev, _lib.query("ir2rgb_grad_check_partial_bytes", tab.nblocks))
    _lib.launch("ir2rgb_grad_check", tab.table, tab.table, tab.blocks, tab.nblocks, part.ptr, st.ptr, None, sc.ptr, math.inf, LR, B1, B2, EPS)
    _lib.launch("ir2rgb_adam_step_checked", tab.table, tab.table, tab.blocks, tab.nblocks, st.ptr)
    torch.cuda.synchronize()
    part.bytes(), sc.bytes()
    return tab.read(), _lib.AdamState.from_buffer_copy(st.bytes())


def _assert_fp64_bounds(what, got, host_scaled, g_ref64, step, dg_rel=0.0):
    """p, m, v against oracle/window_ops_ref.adam fed ``g_ref64`` under oracle/replay_ops.replay_adam's bounds.  ``dg_rel``:
    a relative error of the gradient the kernel works on, |dg| <= dg_rel |g| (0 for an exact unscaling), carried through
    the update: dm = (1-b1) dg;  dv = (1-b2) (2 |g| dg + dg^2);  the denominator sqrt(v)/sqrt(bc2) + eps moves by
    dv / (2 sqrt(v) sqrt(bc2)), and the update by its own size times that over the denominator."""
    b1f, b2f = float(np.float32(B1)), float(np.float32(B2))
    worst = 0.0
    for (n, aligned), arrs, res, gref in zip(SPECS, host_scaled, got, g_ref64):
        p, _, m, v = (t.double().numpy() for t in arrs)
        p1, m1, v1, upd, Sm, ss, den = O.adam(p, gref, m, v, LR, b1f, b2f, EPS, step)
        dg = dg_rel * np.abs(gref)
        dm = (1 - b1f) * dg
        dv = (1 - b2f) * (2 * np.abs(gref) * dg + dg * dg)
        bm = 4 * B.U32 * Sm + B.ETA["f32"] + dm
        bv = 4 * B.U32 * v1 + B.ETA["f32"] + dv
        dden = dv / (2 * np.maximum(np.sqrt(v1), 1e-300) * math.sqrt(1 - b2f ** step))
        bp = B.U32 * np.abs(p1) + 16 * B.U32 * upd + ss * bm / den + upd * dden / den + B.ETA["f32"]
        for name, gv, rv, bb in (("m", res[2], m1, bm), ("v", res[3], v1, bv), ("p", res[0], p1, bp)):
            ok, ratio, i, over = B.check_bound(gv.double().numpy(), rv, bb)
            assert ok, f"{what} n={n} aligned={aligned} {name}: {over} elements over the bound (worst {ratio:.3g} at {i})"
            worst = max(worst, ratio)
        assert torch.equal(res[1], arrs[1]), "the gradient was written"
    return worst


@pytest.mark.parametrize("step", [1, 2, 1000])
@pytest.mark.parametrize("k", [8, 16])
def test_scaled_step_power_of_two(dev, k, step):
    scale = 2.0 ** k
    host = _host_arrays(100 + step, step)
    scaled = [[p, g * scale, m, v] for p, g, m, v in host]
    assert all(torch.equal(s[1] / scale, h[1]) for s, h in zip(scaled, host))          # g * 2^k and back: exact
    got, st = _scaled_step(dev, scaled, scale, step)
    assert st.found_inf == 0.0 and st.step == step and _factor_bits(st) == _inv_scale_bits(scale)
    worst = _assert_fp64_bounds(f"scale 2^{k} step {step}", got, scaled, [h[1].double().numpy() for h in host], step)
    ulps = _ulps(_device_coef(st), _host_coef(step))
    equal = int(ulps.max()) == 0
    print(f"scale 2^{k} step {step}: worst err/bound {worst:.3g}; device coefficients", "EQUAL the host's" if equal
          else f"differ from the host's by {ulps.tolist()} ulp")
    if step == 1:
        assert equal, "pow(b, 1) = b: the coefficients of step 1 must be the host's"
    assert ulps.max() <= 1, "a coefficient is more than 1 ulp of float from the host's"
    if equal:       # then the whole step is ir2rgb_adam_step's on the pre-divided gradient, bit for bit
        plain = _Table(dev, host)
        _lib.launch("ir2rgb_adam_step", plain.table, plain.table, plain.blocks, plain.nblocks, LR, B1, B2, EPS, step)
        torch.cuda.synchronize()
        bad = [(n, aligned, name, int((x.view(torch.int32) != y.view(torch.int32)).sum()))
               for (n, aligned), a, b in zip(SPECS, got, plain.read())
               for name, x, y in zip("pmv", (a[0], a[2], a[3]), (b[0], b[2], b[3])) if not torch.equal(x.view(torch.int32), y.view(torch.int32))]
        assert not bad, f"not bit-identical to ir2rgb_adam_step on g / 2^{k} (n, aligned, array, elements): {bad}"


@pytest.mark.parametrize("step", [1, 14])
def test_scaled_step_scale_1000(dev, step):
    """A scale that is no power of two: inv_scale is a rounded reciprocal and g * inv_scale a rounded product, two
    roundings of 2^-24 relative each on the gradient the update sees."""
    scale = 1000.0
    host = _host_arrays(200 + step, step)
    scaled = [[p, g * scale, m, v] for p, g, m, v in host]
    got, st = _scaled_step(dev, scaled, scale, step)
    assert st.found_inf == 0.0 and st.step == step and _factor_bits(st) == _inv_scale_bits(scale)
    worst = _assert_fp64_bounds(f"scale 1000 step {step}", got, scaled, [s[1].double().numpy() / scale for s in scaled], step,
                                dg_rel=2 * 2.0 ** -24)
    print(f"scale 1000 step {step}: worst err/bound {worst:.3g}")


# ---------------------------------------------------------------------------------------------------------------------
# FusedAdam.step(scaler), LossScaler
def _toy(dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter((torch.randn(n, generator=g) * 0.05).to(dev)) for n in (5, 8193, 100, 3 * 8192)]


def _set_grads(params, scale, seed):
    g = torch.Generator().manual_seed(seed)
    for p in params:
        p.grad = (torch.randn(p.numel(), generator=g) * 0.01 * scale).to(p.device)


@pytest.mark.parametrize("interval", [2000, 0])
def test_overflow_skips_the_step_and_moves_the_scale(dev, interval):
    params = _toy(dev)
    opt = OP.FusedAdam(params, lr=LR, betas=(B1, B2))
    scaler = OP.LossScaler(dev, init_scale=256.0, growth_interval=interval)
    # step 1, clean: the bits of a plain optimizer fed the divided gradient (the coefficients of step 1 are the host's)
    twin_params = [torch.nn.Parameter(p.detach().clone()) for p in params]
    twin = OP.FusedAdam(twin_params, lr=LR, betas=(B1, B2))
    _set_grads(params, 256.0, 1)
    _set_grads(twin_params, 1.0, 1)
    assert all(torch.equal(a.grad / 256.0, b.grad) for a, b in zip(params, twin_params))
    before = [p.detach().clone() for p in params]
    opt.step(scaler)
    scaler.update([opt])
    twin.step()
    assert all(not torch.equal(a, p) for a, p in zip(before, params)), "a clean step must move every parameter"
    assert all(torch.equal(a, b) for a, b in zip(params, twin_params))
    assert torch.equal(opt.exp_avg, twin.exp_avg) and torch.equal(opt.exp_avg_sq, twin.exp_avg_sq)
    g_norm = math.sqrt(sum(float(p.grad.double().pow(2).sum()) for p in twin_params))
    assert abs(scaler.stats()["grad_norms"][0] - g_norm) <= 1e-12 * g_norm and scaler.stats()["skipped"] == 0
    # an inf in the middle of a whole chunk: nothing moves, the step count stays, the scale backs off (unless static)
    snap = [p.detach().clone() for p in params], opt.exp_avg.clone(), opt.exp_avg_sq.clone()
    versions = [p._version for p in params]
    _set_grads(params, 256.0, 2)
    params[1].grad[4000] = float("inf")
    opt.step(scaler)
    scaler.update([opt])
    assert all(torch.equal(a, p) for a, p in zip(snap[0], params)) and torch.equal(snap[1], opt.exp_avg) and \
        torch.equal(snap[2], opt.exp_avg_sq), "a skipped step wrote p, m or v"
    assert int(opt.scaled_state()[0].item()) == 1 and opt.grad_stats()[0] is True
    assert all(p._version > v for p, v in zip(params, versions))          # (increment_version stays as it is)
    stats = scaler.stats()
    assert stats["skipped"] == 1 and stats["scale"] == (128.0 if interval else 256.0) and len(stats["grad_norms"]) == 1
    sd = opt.state_dict()
    assert opt.step_count == 1 and all(int(s["step"]) == 1 for s in sd["state"].values())
    # the next clean step is step 2
    _set_grads(params, stats["scale"], 3)
    opt.step(scaler)
    scaler.update([opt])
    assert opt.state_dict()["state"][0]["step"].item() == 2.0 and opt.grad_stats()[0] is False
    assert all(not torch.equal(a, p) for a, p in zip(snap[0], params))
    # a plain step after loss-scaled ones takes the count back to the host
    opt.step()
    assert opt.step_count == 3
    # the scaler's state survives a round trip
    other = OP.LossScaler(dev)
    other.load_state_dict(scaler.state_dict())
    assert other.state_dict() == scaler.state_dict() and torch.equal(other.state, scaler.state)


def test_update_kernel_follows_the_reference_rule(dev):
    """loss_scale_update_kernel over three optimizer states against loss_scale_update_reference (itself held to
    torch._amp_update_scale_ by tests/test_loss_scale_cpu.py): growth at the interval, back-off, a refused growth."""
    nb = _lib.query("ir2rgb_loss_scale_state_bytes", 0)
    for init, growth, backoff, interval, seed in ((1024.0, 2.0, 0.5, 3, 0), (float(np.float32(3e38)), 2.0, 0.5, 2, 1),
                                                  (1000.0, 1.5, 0.25, 2, 2), (4096.0, 2.0, 0.5, 0, 3)):
        blocks = [_Banded(dev, nb, _lib.AdamState(step=5)) for _ in range(3)]
        table = torch.tensor([b.ptr for b in blocks], dtype=torch.int64, device=dev)
        sc = _scaler_block(dev, init)
        s_ref, t_ref, skipped = torch.tensor([init]), torch.zeros(1, dtype=torch.int32), 0
        g = torch.Generator().manual_seed(seed)
        for w in range(24):
            flags = (torch.rand(3, generator=g) < 0.15).float()
            for b, f in zip(blocks, flags.tolist()):
                b.buf[BAND + 8] = int(np.float32(f).view(np.int32))        # found_inf, word 8 of ir2rgb_adam_state
            _lib.launch("ir2rgb_loss_scale_update", table, sc.ptr, table, 3, growth, backoff, interval)
            inv_ref, sk = OP.loss_scale_update_reference(s_ref, t_ref, flags, growth, backoff, interval)
            skipped += sk
            got = _lib.LossScaleState.from_buffer_copy(sc.bytes())
            want = _lib.LossScaleState(scale=s_ref.item(), inv_scale=inv_ref.item(), growth_tracker=t_ref.item(), skipped=skipped)
            assert bytes(got) == bytes(want), (w, flags.tolist(), got.scale, s_ref.item(), got.growth_tracker, got.skipped)
        for b in blocks:
            b.bytes()
    assert _lib.AdamState.found_inf.offset == 32


def test_scale_step_update_never_synchronise(dev):
    params = _toy(dev, 3)
    opt = OP.FusedAdam(params, lr=LR, betas=(B1, B2))
    scaler = OP.LossScaler(dev, init_scale=2.0 ** 10)
    x = [torch.randn(p.numel(), device=dev) for p in params]

    def window():
        opt.zero_grad()
        loss = sum((p * t).sum() for p, t in zip(params, x))
        (loss * scaler.scale_tensor).backward()
        opt.step(scaler)
        scaler.update([opt])

    for _ in range(3):          # allocations, the state blocks, both pinned table copies
        window()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(3):
            window()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert scaler.stats()["skipped"] == 0 and opt.state_dict()["state"][0]["step"].item() == 6.0


# ---------------------------------------------------------------------------------------------------------------------
# the trainer
def _trainer(dev, dtype, **kw):
    from ir2rgb_amd import vid2vid as V
    tr = V.Vid2VidTrainer(dev, compute_dtype=dtype, first_layer_gen_filters=64, build_flow_net=False, **kw)
    tr.flow_net = stub_flow_and_conf
    return tr


def _optimizers(tr):
    return [tr.optimizer_G, tr.optimizer_D] + list(tr.optimizer_D_T)


def _state(tr):
    """Every parameter and both moment buffers of every optimizer, cloned."""
    return [[torch.cat([p.detach().flatten() for p in o.params]), o.exp_avg.clone(), o.exp_avg_sq.clone()] for o in _optimizers(tr)]


def _grads(tr):
    """Per optimizer the gradients as the step saw them, flattened in parameter order (None: no backward pass reached it)."""
    out = []
    for fg in [tr.grads_G, tr.grads_D] + list(tr.grads_DT):
        out.append(None if any(p.grad is None for p in fg.params) else torch.cat([p.grad.detach().flatten() for p in fg.params]))
    return out


def test_trainer_bf16_static_scale_is_exactly_linear(dev):
    from ir2rgb_amd import vid2vid as V
    A, Bs = V.synthetic_sequence(4, 64, 128, 3, dev)
    runs = {}
    for name, kw in (("plain", {}), ("scaled", {"loss_scale": 256.0})):
        tr = _trainer(dev, torch.bfloat16, **kw)
        out0 = tr.train_window(A[:, 0:3], Bs[:, 0:3])
        g0 = _grads(tr)
        out1 = tr.train_window(A[:, 1:4], Bs[:, 1:4])
        runs[name] = (g0, _state(tr), [out0, out1], tr)
    tr = runs["scaled"][3]
    assert tr.loss_scaler is not None and runs["plain"][3].loss_scaler is None
    assert tr.loss_scaler.stats()["skipped"] == 0 and tr.loss_scaler.stats()["scale"] == 256.0
    excluded = total = 0
    for i, (a, b) in enumerate(zip(runs["plain"][0], runs["scaled"][0])):
        assert (a is None) == (b is None)
        if a is None:
            continue
        tiny = (a != 0) & (a.abs() < 2.0 ** -100)
        excluded += int(tiny.sum())
        total += a.numel()
        keep = ~tiny
        same = (a[keep] * 256.0).view(torch.int32) == b[keep].view(torch.int32)
        same |= (a[keep] == 0) & (b[keep] == 0)
        assert bool(same.all()), f"optimizer {i}: {int((~same).sum())} of {a.numel()} gradient elements are not 2^8 x the unscaled ones"
    print("elements with 0 < |g| < 2^-100, left out:", excluded, "of", total, "share", excluded / total)
    assert excluded <= 1e-4 * total
    for i, (sa, sb) in enumerate(zip(runs["plain"][1], runs["scaled"][1])):
        for name, x, y in zip(("parameters", "exp_avg", "exp_avg_sq"), sa, sb):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), f"optimizer {i}: {name} differ after two windows"
    for w in range(2):
        la, lb = runs["plain"][2][w], runs["scaled"][2][w]
        assert la.keys() == lb.keys()
        for k in la:
            assert la[k].item() == lb[k].item(), (w, k, la[k].item(), lb[k].item())


def test_trainer_f16_dynamic_scale_recovers_from_overflow(dev):
    from ir2rgb_amd import vid2vid as V
    scaler = OP.LossScaler(dev, init_scale=2.0 ** 30)
    tr = _trainer(dev, torch.float16, loss_scale=scaler)
    assert tr.loss_scaler is scaler
    A, Bs = V.synthetic_sequence(12, 64, 128, 3, dev)
    start = _state(tr)
    scale, skipped, passed = 2.0 ** 30, 0, None
    for w in range(30):
        before = _state(tr)
        i = w % 10
        tr.train_window(A[:, i:i + 3], Bs[:, i:i + 3])
        stats = scaler.stats()
        active = _optimizers(tr)[:len(stats["grad_norms"])]
        found = [o.grad_stats()[0] for o in active]
        for o, f, b, a in zip(active, found, before, _state(tr)):
            if f:
                assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(b, a)), "a skipped optimizer changed"
        if any(found):
            skipped += 1
            scale *= 0.5
        assert stats["scale"] == scale and stats["skipped"] == skipped
        if not any(found):
            passed = w
            break
    print("first window without overflow:", passed, "scale", scale, "gradient norms", stats["grad_norms"])
    assert passed is not None and passed >= 1, "the first windows must overflow at 2^30, and one of 30 must pass"
    assert skipped == round(math.log2(2.0 ** 30 / scale))
    for o, s0, s1 in zip(active, start, _state(tr)):
        assert all(bool(torch.isfinite(t).all()) for t in s1)
        assert not torch.equal(s0[0], s1[0]), "the parameters have not moved"
    assert all(math.isfinite(n) for n in stats["grad_norms"])


def test_small_losses_f16_discriminator(dev):
    """A loss 2^-14 of its size through the 5-layer discriminator in f16: with a static scale of 2^14 the parameter
    gradients are the ordinary run's bit for bit; without it the activation gradients fall under f16's range."""
    from ir2rgb_amd import networks as N
    from ir2rgb_amd.losses import fused_losses
    torch.manual_seed(22)
    d = N.build_discriminator_module(6, 64, 3, "batch", 2, True).train().to(dev)
    assert sum(isinstance(m, torch.nn.Conv2d) for m in d.modules()) == 2 * 5
    d.compute_dtype = torch.float16
    x = smooth((2, 6, 64, 128), 5).to(dev)
    scaler = OP.LossScaler(dev, init_scale=2.0 ** 14, growth_interval=0)

    def grads(factor, scale_tensor):
        d.zero_grad(set_to_none=True)
        loss = fused_losses([("mse", sc[-1], 1.0, 1.0, 0) for sc in d(x)], 1, torch.float16)[0]
        if factor is not None:
            loss = loss * factor
        if scale_tensor is not None:
            loss = loss * scale_tensor
        loss.backward()
        got = [p.grad.detach().flatten().clone() for p in d.parameters() if p.grad is not None]
        assert len(got) >= 2 * 5                     # (every convolution weight at least)
        return torch.cat(got)

    ordinary = grads(None, None)
    assert torch.equal(ordinary, grads(None, None)), "the ordinary run does not repeat bit for bit"
    rescued = grads(2.0 ** -14, scaler.scale_tensor)
    assert torch.equal(rescued.view(torch.int32), ordinary.view(torch.int32))
    lost = grads(2.0 ** -14, None) * 2.0 ** 14
    err = ((lost.double() - ordinary.double()).norm() / ordinary.double().norm()).item()
    print("small loss without the scaler: relative L2 error of the parameter gradients", err)
    assert not torch.equal(lost, ordinary)


def test_f16_window_golden_under_dynamic_scale(dev, golden_dir, monkeypatch):
    """tests/test_harness_gpu.py's golden comparison itself, bounds and all, with ``loss_scale="dynamic"`` (2^16) as the
    trainer's default.  The case is the one whose learning rate is 0: every one of its windows is held to window-0
    accuracy and no result depends on whether a window's step was skipped.  The comparison reads ``p.grad``, so the
    gradients are unscaled in place once the window (steps included) is over."""
    import test_harness_gpu as H
    from ir2rgb_amd import vid2vid as V
    monkeypatch.setitem(V.DEFAULTS, "loss_scale", "dynamic")
    seen = []
    inner = V.Vid2VidTrainer.train_window

    def train_window(self, *a):
        inv = 1.0 / self.loss_scaler.scale_tensor.clone()
        out = inner(self, *a)
        for o in _optimizers(self):
            for p in o.params:
                if p.grad is not None:
                    p.grad.mul_(inv)
        seen.append(self)
        return out

    monkeypatch.setattr(V.Vid2VidTrainer, "train_window", train_window)
    H.test_training_windows_vs_reference_golden(dev, golden_dir, "ngf64_64x128_lr0", torch.float16)
    assert seen and all(t is seen[0] for t in seen)
    st = seen[0].loss_scaler.state_dict()
    print("dynamic scale over the golden's windows:", st)
    # (the tracker counts the clean windows since the last skipped one)
    assert st["scale"] == 2.0 ** 16 * 0.5 ** st["skipped"] and st["growth_tracker"] <= len(seen) - st["skipped"]
