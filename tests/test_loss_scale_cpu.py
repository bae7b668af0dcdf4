"""CPU side of dynamic loss scaling (ir2rgb_amd.optim): the plain-torch restatements the kernels are tested against are
themselves held to torch's own AMP operators, the trainer's ``loss_scale`` option is validated before anything is built,
and the device state blocks have the size the ctypes structs say.  No GPU."""
import ctypes

import pytest
import torch

from ir2rgb_amd import _lib
from ir2rgb_amd import optim as O


def _torch_update(scale, tracker, found, growth, backoff, interval):
    torch._amp_update_scale_(scale, tracker, torch.tensor([1.0 if found else 0.0]), growth, backoff, interval)


def _run_both(seq, init, growth, backoff, interval):
    """The same found / not-found sequence through torch._amp_update_scale_ and the restatement -> per-window states."""
    s_t, t_t = torch.tensor([init], dtype=torch.float32), torch.zeros(1, dtype=torch.int32)
    s_r, t_r = s_t.clone(), t_t.clone()
    trace, skipped = [], 0
    for found in seq:
        _torch_update(s_t, t_t, found, growth, backoff, interval)
        inv, sk = O.loss_scale_update_reference(s_r, t_r, torch.tensor([0.0, 1.0 if found else 0.0]), growth, backoff, interval)
        skipped += sk
        assert s_r.view(torch.int32).item() == s_t.view(torch.int32).item(), (found, s_r.item(), s_t.item())
        assert t_r.item() == t_t.item()
        assert inv.dtype == torch.float32 and inv.item() == float(torch.tensor(1.0 / float(s_r.item()), dtype=torch.float64).float())
        trace.append((s_r.item(), t_r.item()))
    assert skipped == sum(bool(f) for f in seq)
    return trace


@pytest.mark.parametrize("growth,backoff,interval", [(2.0, 0.5, 3), (1.5, 0.25, 2), (3.0, 0.75, 1), (2.0, 0.5, 2000)])
def test_update_reference_equals_torch_on_random_sequences(growth, backoff, interval):
    g = torch.Generator().manual_seed(interval)
    for trial in range(20):
        seq = (torch.rand(60, generator=g) < (0.05, 0.3, 0.7)[trial % 3]).tolist()
        _run_both(seq, float(2.0 ** (trial % 24)), growth, backoff, interval)


def test_update_reference_growth_backoff_and_refused_growth():
    # growth exactly at the interval, not before
    tr = _run_both([False, False, False, False], 1024.0, 2.0, 0.5, 3)
    assert tr == [(1024.0, 1), (1024.0, 2), (2048.0, 0), (2048.0, 1)]
    # a back-off resets the tracker: the next growth is a whole interval away
    tr = _run_both([False, False, True, False, False, False], 1024.0, 2.0, 0.5, 3)
    assert tr == [(1024.0, 1), (1024.0, 2), (512.0, 0), (512.0, 1), (512.0, 2), (1024.0, 0)]
    # a growth that would reach inf is refused, and the tracker starts over all the same
    big = float(torch.finfo(torch.float32).max) / 1.5
    tr = _run_both([False, False, False], big, 2.0, 0.5, 2)
    assert tr == [(pytest.approx(big), 1), (pytest.approx(big), 0), (pytest.approx(big), 1)]


def test_update_reference_static_scale_never_moves():
    s, t = torch.tensor([1000.0]), torch.zeros(1, dtype=torch.int32)
    skipped = 0
    for found in (False, True, True, False):
        inv, sk = O.loss_scale_update_reference(s, t, torch.tensor([float(found)]), 2.0, 0.5, 0)
        skipped += sk
        assert s.item() == 1000.0 and t.item() == 0 and inv.item() == float(torch.tensor(1e-3, dtype=torch.float64).float())
    assert skipped == 2


@pytest.mark.parametrize("plant", [None, float("inf"), float("-inf"), float("nan"), 3e38])
def test_grad_check_reference_agrees_with_torch_amp(plant):
    g = torch.Generator().manual_seed(5)
    grads = [torch.randn(n, generator=g) * 100.0 for n in (1, 3, 4, 5, 1000)]
    if plant is not None:
        grads[3][2] = plant
        if plant == 3e38:
            grads[4].fill_(3e38)
    inv = torch.tensor(1.0 / 1000.0, dtype=torch.float32)
    found, sumsq, unscaled = O.grad_check_reference(grads, inv)
    theirs = [x.clone() for x in grads]
    found_t = torch.zeros(1)
    torch._amp_foreach_non_finite_check_and_unscale_(theirs, found_t, inv)
    assert found.item() == found_t.item() == (0.0 if plant in (None, 3e38) else 1.0)     # 3e38 is finite: its square is not a float
    for a, b in zip(unscaled, theirs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))                 # same bits, NaN included
    if not found.item():
        want = sum((x.double() ** 2).sum() for x in theirs)
        assert sumsq.dtype == torch.float64 and torch.isfinite(sumsq)
        assert abs(sumsq.item() - want.item()) <= 1e-6 * want.item()     # (theirs were rounded to fp32 after unscaling)


def test_loss_scale_option_is_validated_before_anything_is_built(monkeypatch):
    from ir2rgb_amd import networks, vid2vid as V

    def no_build(*a, **k):
        raise AssertionError("a network was built before the option was refused")
    monkeypatch.setattr(networks, "build_generator_module", no_build)
    cpu = torch.device("cpu")
    for bad in ("static", "Dynamic", -1.0, 0, float("inf"), float("nan"), True, [256.0], 1e-50):
        with pytest.raises(ValueError, match="loss.scale"):
            V.Vid2VidTrainer(cpu, loss_scale=bad)
    for good in (256.0, 2 ** 16, "dynamic"):
        with pytest.raises(ValueError, match="fused_adam"):
            V.Vid2VidTrainer(cpu, loss_scale=good, fused_adam=False)
        assert O.check_loss_scale_option(good, True) in ("static", "dynamic")
    assert O.check_loss_scale_option(None, False) == "none" and V.DEFAULTS["loss_scale"] is None
    with pytest.raises(AssertionError, match="a network was built"):       # the default gets as far as building
        V.Vid2VidTrainer(cpu)
    with pytest.raises(ValueError, match="GPU only"):
        O.LossScaler(cpu)
    for kw in (dict(growth_factor=0.5), dict(backoff_factor=1.5), dict(backoff_factor=0.0), dict(growth_factor=1.1),
               dict(growth_interval=-1), dict(growth_interval=2.5), dict(init_scale=0.0)):
        with pytest.raises(ValueError, match="loss scale"):
            O.check_scaler_arguments(**{**dict(scale=kw.pop("init_scale", 65536.0), growth_factor=2.0, backoff_factor=0.5,
                                               growth_interval=2000), **kw})


def test_state_block_sizes_match_the_ctypes_structs():
    from ir2rgb_amd import build
    build.build()
    assert _lib.query("ir2rgb_loss_scale_state_bytes", 0) == ctypes.sizeof(_lib.AdamState) == 48
    assert _lib.query("ir2rgb_loss_scale_state_bytes", 1) == ctypes.sizeof(_lib.LossScaleState) == 16
    assert _lib.AdamState.grad_sumsq.offset % 8 == 0 and _lib.AdamState.found_inf.offset == 32
    with pytest.raises(ValueError, match="loss_scale_state_bytes"):
        _lib.query("ir2rgb_loss_scale_state_bytes", 2)
    chunk_rows = _lib.query("ir2rgb_grad_check_partial_bytes", 7)
    assert chunk_rows == 7 * 16 and _lib.query("ir2rgb_grad_check_partial_bytes", 0) == 16
    # argument checks return before any launch (no GPU here): NULL pointers, misaligned state blocks, bad factors
    lib = _lib.lib()
    buf = torch.zeros(64, dtype=torch.float64)
    p = buf.data_ptr()
    assert p % 8 == 0
    inf = float("inf")
    assert lib.ir2rgb_grad_check(None, p, 1, p, p, None, p, inf, 2e-4, 0.5, 0.999, 1e-8, None) == -1
    assert lib.ir2rgb_grad_check(p, p, 1, p, p, None, p, inf, 2e-4, 1.0, 0.999, 1e-8, None) == -1
    assert lib.ir2rgb_grad_check(p, p, 1, p, p + 4, None, p, inf, 2e-4, 0.5, 0.999, 1e-8, None) == -3
    assert lib.ir2rgb_grad_check(p, p, 1, p + 4, p, None, p, inf, 2e-4, 0.5, 0.999, 1e-8, None) == -3
    assert lib.ir2rgb_adam_step_checked(p, p, -1, p, None) == -1
    assert lib.ir2rgb_adam_step_checked(p, p, 1, p + 4, None) == -3
    assert lib.ir2rgb_adam_step_checked(p, p, 0, p, None) == 0
    assert lib.ir2rgb_loss_scale_update(p, p, 9, 2.0, 0.5, 2000, None) == -1
    assert lib.ir2rgb_loss_scale_update(p, p, 1, 0.5, 0.5, 2000, None) == -1
    assert lib.ir2rgb_loss_scale_update(p, p, 1, 2.0, 0.5, -1, None) == -1
    assert lib.ir2rgb_loss_scale_update(p + 2, p, 1, 2.0, 0.5, 2000, None) == -3
    assert lib.ir2rgb_loss_scale_update(p, p, 0, 2.0, 0.5, 2000, None) == 0
