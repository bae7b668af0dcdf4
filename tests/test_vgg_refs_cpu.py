"""The references and checks of oracle/vgg_ref.py, on the CPU alone (run with -s for the figures).

* the inputs meet the conditions the GPU tests rely on: every term holds at least 5 % of the fp64 loss, nothing is
  non-finite, and in the emulation fewer than 1 % of the non-zero gradient elements of any stage lie below the smallest
  normal number of the format (2^-14 for f16, whose backward pass is rooted at 2^12; bf16 has fp32's range, so there
  the threshold is 2^-126 and the root 1);
* the fp64 chain is torch's own ``slice{s}`` modules in fp64 on the same rounded operands, to 1e-12;
* every check the GPU file asserts accepts the unfaulted emulation -- also with the input channels of every
  convolution permuted, i.e. another summation order -- and each planted fault of vgg_ref.FAULTS is rejected by the
  checks that look at what it breaks (EXPECT below; the whole matrix of ratios is printed).

The drift checks are calibrated on the unfaulted emulation's own distance from fp64 (vgg_ref.noise_level, times
vgg_ref.DRIFT_FACTOR): the permuted emulation checked here is a further draw of the same rounding noise, so it shows the
spread the factor has to cover.
"""
import copy
import math

import pytest
import torch

from oracle import bounds as B
from oracle import vgg_ref as R

CASES = [(shape, fmt) for shape in R.SHAPES for fmt in R.FORMATS]
IDS = [f"{s[0]}x{s[2]}x{s[3]}-{f}" for s, f in CASES]

# the checks that must reject each fault (a gross feature fault also has to exceed the drift margin on the features)
EXPECT = {
    "no_bias_conv4_1": ("stage_fwd", "drift_features"),
    "leaky_conv3_2": ("stage_fwd", "stage_bwd"),        # (1 % of the negative half: inside bf16's drift margin)
    "no_mask_conv3_3": ("stage_bwd",),
    "avg_pool3": ("pools", "drift_features"),
    "w1_x2": ("loss_value", "loss_grads"),
    "w3_x1.25": ("loss_value", "loss_grads"),
    "drop5": ("loss_value", "loss_grads"),
    "wrong_n": ("loss_grads",),
}

_CACHE = {}


def _vgg():
    if "vgg" not in _CACHE:
        from ir2rgb_amd.vgg import Vgg19
        _CACHE["vgg"] = R.init_weights(Vgg19())
    return _CACHE["vgg"]


def _case(shape, fmt):
    key = (shape, fmt)
    if key not in _CACHE:
        vgg = _vgg()
        x, y = R.images(shape)
        ref = R.reference64(vgg, x, y, R.FORMATS[fmt])
        rec, grad = R.emulated(vgg, x, y, fmt)
        noise = R.noise_level(vgg, x, y, fmt, ref)
        _CACHE[key] = (vgg, x, y, ref, rec, grad, noise)
    return _CACHE[key]


@pytest.mark.parametrize("shape,fmt", CASES, ids=IDS)
def test_input_conditions(shape, fmt):
    vgg, x, y, ref, rec, grad, _ = _case(shape, fmt)
    shares = [t / ref["loss"] for t in ref["terms"]]
    print(f"\n{shape} {fmt}: term shares of the fp64 loss " + " ".join(f"{100 * s:.1f}%" for s in shares))
    assert min(shares) >= 0.05
    assert all(torch.isfinite(t).all() for t in ref["fx"] + ref["fy"] + [ref["grad"]])
    assert torch.isfinite(grad).all() and math.isfinite(rec.loss["value"])
    worst = 0.0
    for st in rec.stages[:13]:
        for g in (st["gz"], st["gx"]):
            assert torch.isfinite(g).all() and torch.isfinite(st["z"]).all()
            nz = g[g != 0].abs()
            worst = max(worst, float((nz < B.ETA[fmt]).float().mean()))
    print(f"{shape} {fmt}: largest share of non-zero stage gradients below the smallest normal: {100 * worst:.3f}%")
    assert worst < 0.01
    for st in rec.stages[13:]:
        assert torch.isfinite(st["z"]).all()


@pytest.mark.parametrize("shape,fmt", CASES, ids=IDS)
def test_fp64_chain_is_torchs_own_modules(shape, fmt):
    vgg, x, y, ref, *_ = _case(shape, fmt)
    dt = R.FORMATS[fmt]
    tv = copy.deepcopy(vgg)
    with torch.no_grad():
        for m in R.convs(tv):
            m.weight.copy_(m.weight.to(dt).float())
    tv = tv.double()
    for img, feats in ((x, ref["fx"]), (y, ref["fy"])):
        h = img.to(dt).double()
        for s in range(1, 6):
            with torch.no_grad():
                h = getattr(tv, f"slice{s}")(h)
            assert R.rel_l2(feats[s - 1], h) <= 1e-12, s


@pytest.mark.parametrize("shape,fmt", CASES, ids=IDS)
def test_emulation_noise_floor(shape, fmt):
    """The emulated chain against the fp64 chain (printed; seen: bf16 features 1.7e-3 .. 4.6e-3, f16 2.1e-4 .. 5.9e-4,
    bf16 gradient 0.27 at 35 x 53 -- L1 signs and ReLU masks flip).  Rounding to half cannot move a feature map by more
    than a few unit roundoffs per layer: 13 layers * 4 u is the coarse ceiling asserted."""
    vgg, x, y, ref, rec, grad, noise = _case(shape, fmt)
    print(f"\n{shape} {fmt}: emulation vs fp64, per-slice relative L2 " + " ".join(f"{d:.2e}" for d in noise[0])
          + f"; image gradient {noise[1]:.3f}; loss {abs(rec.loss['value'] - ref['loss']) / ref['loss']:.2e}")
    assert max(noise[0]) <= 13 * 4 * B.U_OUT[fmt]
    assert abs(rec.loss["value"] - ref["loss"]) <= 13 * 4 * B.U_OUT[fmt] * ref["loss"]


@pytest.mark.parametrize("shape,fmt", CASES, ids=IDS)
def test_checks_accept_the_unfaulted_emulation(shape, fmt):
    vgg, x, y, ref, rec, grad, noise = _case(shape, fmt)
    plain, detail = R.run_checks(rec, grad, ref, noise, fmt)
    print(f"\n{shape} {fmt} plain:    " + " ".join(f"{k} {v:.3g}" for k, v in plain.items()))
    print("  worst forward ratio per stage:  " + " ".join(f"{v:.3f}" for v in detail["fwd"]))
    print("  worst backward ratio per stage: " + " ".join(f"{v:.3f}" for v in detail["bwd"]))
    assert all(v <= 1.0 for v in plain.values()), plain
    rec2, grad2 = R.emulated(vgg, x, y, fmt, perm_seed=R.NOISE_DRAWS + 3)       # (an order the calibration did not use)
    perm, detail2 = R.run_checks(rec2, grad2, ref, noise, fmt)
    print(f"{shape} {fmt} permuted: " + " ".join(f"{k} {v:.3g}" for k, v in perm.items()))
    print("  drift, permuted / calibration level: features " + " ".join(f"{a / b:.3f}" for a, b in zip(detail2["drift_features"], noise[0]))
          + f"; gradient {detail2['drift_gradient'] / noise[1]:.3f}")
    assert all(v <= 1.0 for v in perm.values()), perm


@pytest.mark.parametrize("fault", list(R.FAULTS))
@pytest.mark.parametrize("shape,fmt", CASES, ids=IDS)
def test_checks_reject_the_planted_fault(shape, fmt, fault):
    vgg, x, y, ref, rec0, _, noise = _case(shape, fmt)
    rec, grad = R.emulated(vgg, x, y, fmt, fault=fault)
    got, detail = R.run_checks(rec, grad, ref, noise, fmt)
    moved = abs(rec.loss["value"] - rec0.loss["value"]) / rec0.loss["value"]
    print(f"\n{shape} {fmt} {fault} ({R.FAULTS[fault]}): loss moved {moved:.2e}; "
          + " ".join(f"{k} {v:.3g}" for k, v in got.items()))
    for name in EXPECT[fault]:
        assert got[name] > 1.0, (fault, name, got[name])
