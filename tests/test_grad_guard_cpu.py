"""CPU side of guarded optimizer steps (ir2rgb_amd.optim.GradGuard, grad_guard_reference, the trainer's ``max_grad_norm``):
the option is validated before anything is built, the restated rule is held to ``torch.nn.utils.clip_grad_norm_`` and to
exact cases, and ``decision_errors`` -- the comparison tests/test_grad_guard_gpu.py applies to what the device decided --
is shown to reject five faulty rules.  No GPU."""
import ctypes
import math

import numpy as np
import pytest
import torch

from ir2rgb_amd import _lib
from ir2rgb_amd import optim as O
from ir2rgb_amd.training import loss_names

F = np.float32
INF = float("inf")


def f32_bits(x):
    return int(np.array([x], dtype=F).view(np.int32)[0])


def decision_errors(got, grads, max_norm, inv_scale=1.0):
    """The device's decision for ONE optimizer step against the rule -> a list of complaints (empty: accepted).

    ``got``: {"found", "sumsq" (the sum of squares of the stored gradient as the device summed it), "norm", "c", "factor"
    (the fp32 values of ir2rgb_grad_guard_state), "d_step", "d_steps", "d_clipped", "d_skipped" (by how much the
    optimizer's step count and the guard's three counters moved)}.  ``grads``: the stored gradients.

    * found is the reference's; after it nothing advances but ``skipped``.
    * sumsq within 2 n 2^-53 sumsq of the fp64 reference, n the element count: both are sums of exactly representable
      non-negative products in some order, one gamma_n each.
    * norm, c, factor equal, bit for bit as fp32, the rule evaluated in double on the device's own sumsq.
    * clipped moves exactly when c < 1."""
    found, sumsq, _, _, _ = O.grad_guard_reference(grads, max_norm, inv_scale)
    n = sum(int(torch.as_tensor(g).numel()) for g in grads)
    bad = []
    if bool(got["found"]) != found:
        return [f"found {got['found']} but the reference says {found}"]
    if found:
        if (got["d_step"], got["d_steps"], got["d_clipped"], got["d_skipped"]) != (0, 0, 0, 1):
            bad.append(f"a skipped step moved step/steps/clipped/skipped by {got['d_step'], got['d_steps'], got['d_clipped'], got['d_skipped']}")
        return bad
    if not abs(got["sumsq"] - sumsq) <= 2 * n * 2.0 ** -53 * sumsq:
        bad.append(f"sumsq {got['sumsq']!r} is not within 2 n 2^-53 of {sumsq!r}")
    norm, c, factor = O.grad_guard_rule(got["sumsq"], max_norm, inv_scale)
    for name, want in (("norm", norm), ("c", c), ("factor", factor)):
        if f32_bits(got[name]) != f32_bits(want):
            bad.append(f"{name} {float(got[name])!r} is not fp32({want!r})")
    if (got["d_step"], got["d_steps"], got["d_skipped"]) != (1, 1, 0):
        bad.append(f"a taken step moved step/steps/skipped by {got['d_step'], got['d_steps'], got['d_skipped']}")
    if got["d_clipped"] != int(c < 1.0):
        bad.append(f"clipped moved by {got['d_clipped']} with c {c!r}")
    return bad


def decision_of(grads, max_norm, inv_scale=1.0, rule=None):
    """A decision as a device following ``rule(sumsq, max_norm, inv) -> (norm, c, factor)`` would report it."""
    found, sumsq, _, _, _ = O.grad_guard_reference(grads, max_norm, inv_scale)
    if found:
        return {"found": True, "sumsq": sumsq, "norm": math.nan, "c": 0.0, "factor": 0.0, "d_step": 0, "d_steps": 0,
                "d_clipped": 0, "d_skipped": 1}
    norm, c, factor = (rule or O.grad_guard_rule)(sumsq, max_norm, inv_scale)
    return {"found": False, "sumsq": sumsq, "norm": F(norm), "c": F(c), "factor": F(factor), "d_step": 1, "d_steps": 1,
            "d_clipped": int(c < 1.0), "d_skipped": 0}


def _grads(seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g) * scale for n in (1, 5, 4097, 300)]


# ---------------------------------------------------------------------------------------------------------------------
# arguments
def test_option_is_checked_before_anything_is_built():
    assert O.check_grad_guard_option(None, True) is None and O.check_grad_guard_option(None, False) is None
    assert O.check_grad_guard_option(INF, True) == {"G": INF, "D": INF, "D_T": INF}
    assert O.check_grad_guard_option(2, True) == {"G": 2.0, "D": 2.0, "D_T": 2.0}
    assert O.check_grad_guard_option({"G": 0.5}, True) == {"G": 0.5, "D": INF, "D_T": INF}
    assert O.check_grad_guard_option({"D": 3.0, "D_T": INF}, True) == {"G": INF, "D": 3.0, "D_T": INF}
    assert O.check_grad_guard_option({}, True) == {"G": INF, "D": INF, "D_T": INF}
    for bad in (0, 0.0, -1.0, math.nan, -INF, True, "1", [1.0], 1e-60, {"G": 0.0}, {"G": math.nan}, {"X": 1.0}, {"G": 1.0, "d": 1.0},
                {"D_T": -2.0}, {"D": None}):
        with pytest.raises(ValueError, match="max_grad_norm"):
            O.check_grad_guard_option(bad, True)
    for good in (1.0, INF, {"G": 1.0}):
        with pytest.raises(ValueError, match="fused_adam"):
            O.check_grad_guard_option(good, False)


def test_trainer_refuses_the_option_before_building():
    from ir2rgb_amd import vid2vid as V
    cpu = torch.device("cpu")
    for kw in (dict(max_grad_norm=0.0), dict(max_grad_norm={"Q": 1.0}), dict(max_grad_norm=math.nan),
               dict(max_grad_norm=1.0, fused_adam=False)):
        with pytest.raises(ValueError, match="max_grad_norm"):
            V.Vid2VidTrainer(cpu, build_flow_net=False, **kw)
    assert V.DEFAULTS["max_grad_norm"] is None


def test_grad_guard_arguments():
    with pytest.raises(ValueError, match="FusedAdam"):
        O.GradGuard(torch.optim.Adam([torch.nn.Parameter(torch.zeros(3))]), 1.0)
    for bad in (0.0, -1.0, math.nan, True, None, "inf"):
        with pytest.raises(ValueError, match="max_norm"):
            O.check_max_norm(bad)
    assert O.check_max_norm(INF) == INF and O.check_max_norm(1) == 1.0 and O.check_max_norm(0.1) == float(F(0.1))
    assert ctypes.sizeof(_lib.GradGuardState) == 32
    assert [getattr(_lib.GradGuardState, n).offset for n in ("grad_norm", "clip_coef", "factor", "steps", "clipped", "skipped")] == \
        [0, 4, 8, 12, 16, 20]


def test_loss_names_with_gradient_norms():
    assert loss_names(2, grad_norms=False) == loss_names(2) and len(loss_names(2)) == 21
    names = loss_names(2, grad_norms=True)
    assert names[:21] == loss_names(2) and names[21:] == ["GN_G", "GN_D", "GN_D_T0", "GN_D_T1"] and len(names) == 25 <= 32


# ---------------------------------------------------------------------------------------------------------------------
# the rule
@pytest.mark.parametrize("inv_scale", [1.0, 2.0 ** -12, 1.0 / 1000.0])
@pytest.mark.parametrize("ratio", [0.3, 0.999, 1.5, INF])
def test_reference_is_clip_grad_norm_after_the_unscaling(ratio, inv_scale):
    inv = float(F(inv_scale))
    stored = _grads(7, scale=1.0 / inv)
    true_norm = math.sqrt(sum(float((g.double() ** 2).sum()) for g in stored)) * inv
    max_norm = float(F(ratio * true_norm))
    found, sumsq, norm, c, factor = O.grad_guard_reference(stored, max_norm, inv_scale)
    params = [torch.nn.Parameter(torch.zeros(g.numel(), dtype=torch.float64)) for g in stored]
    for p, g in zip(params, stored):
        p.grad = g.double() * inv                                  # unscale ...
    total = torch.nn.utils.clip_grad_norm_(params, max_norm)       # ... then clip, in fp64
    assert not found and abs(norm - float(total)) <= 1e-12 * norm
    for p, g in zip(params, stored):
        want, got = p.grad, g.double() * (inv * c)
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert factor == float(F(inv * c)) and (c < 1.0) == (ratio < 1.0)


def test_exact_cases():
    for k, e in ((4, -1), (16, 3), (1, 0), (64, -20), (256, 20)):
        g = [torch.full((k,), 2.0 ** e)]
        found, sumsq, norm, c, factor = O.grad_guard_reference(g, INF)
        assert (found, sumsq, norm) == (False, k * 4.0 ** e, math.sqrt(k) * 2.0 ** e)
        assert c == 1.0 and factor == 1.0
        found, sumsq, norm, c, factor = O.grad_guard_reference(g, INF, 2.0 ** -12)
        assert norm == math.sqrt(k) * 2.0 ** (e - 12) and c == 1.0 and factor == 2.0 ** -12
    # norm == max_norm: c = x / (x + 1e-6) < 1, which counts as clipped
    g = [torch.full((4,), 0.5)]
    _, _, norm, c, factor = O.grad_guard_reference(g, 1.0)
    assert norm == 1.0 and c == 1.0 / (1.0 + 1e-6) < 1.0 and factor == float(F(c))
    assert decision_of(g, 1.0)["d_clipped"] == 1 and decision_errors(decision_of(g, 1.0), g, 1.0) == []
    # inf and NaN anywhere: found, nothing else
    for special in (INF, -INF, math.nan):
        g = _grads(3)
        g[2][4096] = special
        assert O.grad_guard_reference(g, 1.0)[0] is True and O.grad_guard_reference(g, 1.0)[3:] == (0.0, 0.0)
    g = [torch.full((8,), 3e38)]                # finite although its square is not a float
    assert O.grad_guard_reference(g, 1.0)[0] is False


# ---------------------------------------------------------------------------------------------------------------------
# five faulty rules, each rejected by the comparison the GPU tests apply
def _clip_before_unscaling(sumsq, x, inv):
    c = min(1.0, x / (math.sqrt(sumsq) + 1e-6))         # the scaled norm is compared with max_norm
    return math.sqrt(sumsq) * inv, c, float(F(inv * c))


def _missing_eps(sumsq, x, inv):
    norm = math.sqrt(sumsq) * inv
    c = min(1.0, x / norm)
    return norm, c, float(F(inv * c))


def _unclamped(sumsq, x, inv):
    norm = math.sqrt(sumsq) * inv
    c = x / (norm + 1e-6)
    return norm, c, float(F(inv * c))


def test_the_comparison_accepts_the_rule_and_rejects_five_faulty_ones():
    inv = 2.0 ** -12
    stored = _grads(11, scale=2.0 ** 12)
    true_norm = O.grad_guard_reference(stored, INF, inv)[2]
    lo, hi = float(F(0.3 * true_norm)), float(F(3.0 * true_norm))
    for x in (lo, hi, INF):
        assert decision_errors(decision_of(stored, x, inv), stored, x, inv) == []
        assert decision_errors(decision_of(stored, x), stored, x) == []
    # 1. clipping before unscaling: with a scale of 2^12 the coefficient is 2^12 too small
    assert decision_errors(decision_of(stored, lo, inv, _clip_before_unscaling), stored, lo, inv)
    assert decision_errors(decision_of(stored, hi, inv, _clip_before_unscaling), stored, hi, inv)
    # 2. per-tensor instead of global norm: the device would report one tensor's sum of squares
    per_tensor = decision_of(stored[2:3], lo, inv)
    assert decision_errors(per_tensor, stored, lo, inv)
    # 3. a missing 1e-6: seen where the norm is the threshold (never clipped then) and in c wherever it is resolved in fp32
    g = [torch.full((4,), 0.5)]
    assert decision_errors(decision_of(g, 1.0, 1.0, _missing_eps), g, 1.0)
    assert decision_errors(decision_of(g, 0.25, 1.0, _missing_eps), g, 0.25)
    # 4. c not clamped at 1: a gradient below the threshold is scaled UP
    assert decision_errors(decision_of(stored, hi, inv, _unclamped), stored, hi, inv)
    assert decision_errors(decision_of(stored, INF, inv, _unclamped), stored, INF, inv)
    # 5. the step count advanced on a skipped step
    poisoned = [t.clone() for t in stored]
    poisoned[1][3] = math.nan
    ok = decision_of(poisoned, lo, inv)
    assert decision_errors(ok, poisoned, lo, inv) == []
    assert decision_errors(dict(ok, d_step=1), poisoned, lo, inv)
    # and a missed inf / a false alarm
    assert decision_errors(dict(decision_of(stored, lo, inv), found=True), stored, lo, inv)
    assert decision_errors(dict(decision_of(stored, lo, inv)), poisoned, lo, inv)
