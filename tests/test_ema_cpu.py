"""The generator average's arithmetic and options without a GPU (ir2rgb_amd.optim.ema_reference / ema_beta /
check_ema_option, ir2rgb_amd.checkpoint.network_path).  ema_reference is what tests/test_ema_gpu.py holds csrc/ema.hip to
with tolerance 0, so it is held to an fp64 recurrence here, and planted faults show that a bit comparison sees them."""
import numpy as np
import pytest

from ir2rgb_amd import checkpoint
from ir2rgb_amd import optim as OP

F = np.float32
BETA = 0.999


def test_reference_follows_the_fp64_recurrence():
    """N = 200 updates towards a random p per step.  Bound 4 N 2^-24 M with M = max|p| + max|e0|: three roundings per
    update, each at most 2^-24 M (|e|, |p - e| and |alpha (p - e)| stay below M), the carried error is multiplied by
    1 - alpha <= 1, and the factor 4 rather than 3 covers the second-order terms."""
    rng = np.random.default_rng(5)
    N, size = 200, 4096
    e = (rng.standard_normal(size) * 0.05).astype(F)
    e64 = e.astype(np.float64)
    M = float(np.abs(e).max())
    pmax = 0.0
    for n in range(1, N + 1):
        p = (rng.standard_normal(size) * 0.05).astype(F)
        pmax = max(pmax, float(np.abs(p).max()))
        e = OP.ema_reference(e, p, n, BETA, True)
        assert e.dtype == F
        alpha = float(F(1.0) - OP.ema_beta(n, BETA, True))         # the coefficient is the specified fp32 number
        assert abs(alpha - (1.0 - min(float(F(BETA)), (1.0 + n) / (10.0 + n)))) <= 2.0 ** -24
        e64 = e64 + alpha * (p.astype(np.float64) - e64)
    bound = 4 * N * 2.0 ** -24 * (M + pmax)
    err = float(np.abs(e.astype(np.float64) - e64).max())
    print("ema_reference vs fp64 after", N, "updates: max error", err, "bound", bound)
    assert err <= bound


def test_warmup_ramp():
    assert OP.ema_beta(1, BETA) == F(2) / F(11) and OP.ema_beta(2, BETA) == F(3) / F(12)
    assert OP.ema_beta(1, BETA).dtype == F
    ramp = [OP.ema_beta(n, BETA) for n in range(1, 12000)]
    assert all(a <= b for a, b in zip(ramp, ramp[1:])), "the ramp is not monotone"
    first = next(n for n in range(1, 12000) if F(1 + n) / F(10 + n) >= F(BETA))
    assert 8980 <= first <= 9000                                    # (1 + n) / (10 + n) = 0.999 at n = 8989 in exact arithmetic
    assert all(b < F(BETA) for b in ramp[:first - 1]) and all(b == F(BETA) for b in ramp[first - 1:])
    assert OP.ema_beta(1, BETA, warmup=False) == F(BETA)
    # beyond 2^20 the ramp is off whatever it would give (a decay above it shows that: 1 - 2^-24 > (1 + n) / (10 + n))
    top = float(F(1.0 - 2.0 ** -24))
    assert OP.ema_beta((1 << 20) - 1, top) < F(top) and OP.ema_beta(1 << 20, top) == F(top) and OP.ema_beta((1 << 20) + 3, top) == F(top)
    # p == e leaves e as it is, bit for bit, specials aside
    e = (np.random.default_rng(0).standard_normal(1000)).astype(F)
    assert np.array_equal(OP.ema_reference(e, e.copy(), 3, BETA).view(np.int32), e.view(np.int32))


def _inputs():
    rng = np.random.default_rng(17)
    return (rng.standard_normal(20000) * 0.05).astype(F), (rng.standard_normal(20000) * 0.05).astype(F)


def _faulty(kind, e, p, n, beta):
    alpha = F(F(1.0) - OP.ema_beta(n, beta))
    if kind == "contracted fma":                        # e + alpha * d with the product unrounded
        d = (p - e).astype(F)
        return (e.astype(np.float64) + np.float64(alpha) * d.astype(np.float64)).astype(F)
    if kind == "beta e + alpha p":
        b = OP.ema_beta(n, beta)
        return ((b * e).astype(F) + (alpha * p).astype(F)).astype(F)
    if kind == "alpha of the previous n":
        alpha = F(F(1.0) - OP.ema_beta(n - 1, beta))
        return (e + (alpha * (p - e).astype(F)).astype(F)).astype(F)
    raise AssertionError(kind)


@pytest.mark.parametrize("kind", ["contracted fma", "beta e + alpha p", "alpha of the previous n"])
def test_planted_faults_change_bits(kind):
    """(fp64 holds the product of two floats exactly and the sum of it and a float to far below half an ulp of float, so
    the double evaluation rounded once is the fused multiply-add on all but measure-zero ties.)"""
    e, p = _inputs()
    n = 9                                                # inside the ramp: the previous n has another alpha
    good = OP.ema_reference(e, p, n, BETA)
    bad = _faulty(kind, e, p, n, BETA)
    differing = int((good.view(np.int32) != bad.view(np.int32)).sum())
    print(kind, ":", differing, "of", e.size, "elements differ")
    assert differing >= 1


def test_check_ema_option():
    assert OP.check_ema_option(None) is None
    assert OP.check_ema_option(0.0) == 0.0
    assert OP.check_ema_option(0.999) == float(F(0.999))
    for bad in (1.0, -0.1, float("nan"), "x", True):
        with pytest.raises(ValueError, match="ema_decay"):
            OP.check_ema_option(bad)


def test_trainer_defaults_leave_the_average_off():
    from ir2rgb_amd import vid2vid as V
    assert V.DEFAULTS["ema_decay"] is None and V.DEFAULTS["ema_warmup"] is True
    import torch
    with pytest.raises(ValueError, match="ema_decay"):
        V.Vid2VidTrainer(torch.device("cpu"), ema_decay=1.0)


def test_network_path_of_the_averaged_generator(tmp_path):
    assert checkpoint.network_path(str(tmp_path), "G0_ema", "latest") == str(tmp_path / "latest_net_G0_ema.pth")
