"""The VGG19 perceptual loss (ir2rgb_amd/vgg.py) held to fp64, stage by stage and end to end (run with -s for the figures).

One real ``VGGLoss(vgg)(x, y)`` forward and backward per case runs with ``ir2rgb_amd.vgg.A.conv_stage`` and
``ir2rgb_amd.vgg.fused_losses`` wrapped by oracle.vgg_ref.Recorder, which keeps every stage's input, output, the total
gradient arriving at the output and the gradient sent to the input, and the loss assembly's features, value and
gradients.  Everything asserted is a function of that recording and of CPU references (oracle/vgg_ref.py;
tests/test_vgg_refs_cpu.py shows on the CPU that each check rejects planted faults and accepts the unfaulted emulation):

* every convolution (13 of x, 13 of y) against the fp64 convolution OF ITS RECORDED INPUT, element by element, under
  bounds.bound(ref_pre, S, fmt, 9 Cin + 2); every input gradient against the fp64 adjoint of gz * [z > 0] under
  bounds.bound(ref, S, fmt, 9 Cout + 2) -- the first layer's fp32 image gradient under the two-step bound derived in
  vgg_ref.first_bwd_ref;
* every pooled tensor equals F.max_pool2d of the recorded stage output bit for bit;
* the loss value against sum w_i mean|a_i - b_i| in fp64 of the recorded features under bounds.bound_rw (the loss
  slots' chain and c_term); the gradient handed to each feature is sign(a_i - b_i) * half(gout * w_i / n_i) bit for bit
  and nothing is handed to y's features; and |loss - loss_fp64| <= sum w_i (mean|a'_i - a_i| + mean|b'_i - b_i|) + that
  bound against the fp64 chain's features (a triangle inequality, both sides computed here);
* drift: the per-slice relative L2 of the device features, and of x.grad, against the fp64 chain stay within 1.5 times
  the rounding-emulating chain's own distance from it (vgg_ref.noise_level: the root mean square over eight summation
  orders), computed on the CPU in the same test.  The gradient figure is a NOISE measurement -- L1 signs and ReLU
  masks flip under half rounding, the emulation itself sits at 0.05 .. 0.24 -- and pins little; the stage and loss
  checks above carry the precision.

Shapes: (2, 3, 35, 53) -- N > 1, every pool floors an odd extent (35 -> 17 -> 8 -> 4 -> 2, 53 -> 26 -> 13 -> 6 -> 3)
-- and (1, 3, 17, 19) -- relu4_1 is 2 x 2, relu5_1 a single pixel; bf16 and f16 (backward rooted at 2^12) at both.

Figures of the run this file was written with (MI355X), cases in the order 35x53 bf16, 35x53 f16, 17x19 bf16, 17x19 f16:

    worst err/bound   forward (26 stages)   backward (stages 2..13)   image gradient   loss value
                      0.994 0.932 0.988 0.901   0.987 0.755 0.977 0.788   0.881 0.604 0.837 0.605   8e-4 3e-3 2e-4 1e-3
    (the forward figures near 1 are the output rounding itself: u |ref| is met just above a power of two)

    relative L2 against the fp64 chain, device | emulation (vgg_ref.noise_level), relu1_1 .. relu5_1, then x.grad
    35x53 bf16  1.660e-3 2.743e-3 3.346e-3 4.142e-3 4.761e-3 | 1.660e-3 2.743e-3 3.345e-3 4.166e-3 4.769e-3   0.2453 | 0.2409
    35x53 f16   2.077e-4 3.431e-4 4.209e-4 5.264e-4 6.053e-4 | 2.077e-4 3.431e-4 4.218e-4 5.273e-4 6.128e-4   0.0819 | 0.0858
    17x19 bf16  1.643e-3 2.741e-3 3.422e-3 4.095e-3 3.517e-3 | 1.643e-3 2.743e-3 3.424e-3 3.950e-3 3.608e-3   0.1185 | 0.1255
    17x19 f16   2.122e-4 3.411e-4 4.252e-4 5.255e-4 4.784e-4 | 2.122e-4 3.403e-4 4.213e-4 4.992e-4 4.381e-4   0.0592 | 0.0490

    |loss - loss_fp64| <= right-hand side: 1.6e-4 <= 7.0e-3, 4.1e-5 <= 8.9e-4, 1.0e-5 <= 2.0e-3, 1.2e-5 <= 2.4e-4
"""
import pytest
import torch

from oracle import vgg_ref as R

pytestmark = pytest.mark.gpu

CASES = [(shape, fmt) for shape in R.SHAPES for fmt in R.FORMATS]
IDS = [f"{s[0]}x{s[2]}x{s[3]}-{f}" for s, f in CASES]
_CACHE = {}


def _run(shape, fmt):
    """One device run and its CPU references per case, shared by the tests below and left unchanged."""
    key = (shape, fmt)
    if key not in _CACHE:
        from ir2rgb_amd.vgg import VGGLoss, Vgg19
        dev = torch.device("cuda:0")
        if "vgg" not in _CACHE:
            _CACHE["vgg"] = R.init_weights(Vgg19())
        cpu = _CACHE["vgg"]
        vgg = Vgg19().to(dev)
        vgg.load_state_dict(cpu.state_dict())
        vgg.compute_dtype = R.FORMATS[fmt]
        x, y = R.images(shape)
        xd = x.to(dev).requires_grad_()
        rec, grad = R.device_record(VGGLoss(vgg), xd, y.to(dev), fmt)
        for st in rec.stages:               # the references read the CPU copy of the same parameters
            st["conv"] = R.convs(cpu)[R.convs(vgg).index(st["conv"])]
        ref = R.reference64(cpu, x, y, R.FORMATS[fmt])
        _CACHE[key] = {"rec": rec, "grad": grad, "ref": ref, "noise": R.noise_level(cpu, x, y, fmt, ref)}
    return _CACHE[key]


@pytest.mark.parametrize("shape,fmt", CASES, ids=IDS)
def test_every_convolution_forward(shape, fmt):
    rec = _run(shape, fmt)["rec"]
    assert len(rec.stages) == 26 and all(torch.isfinite(st["z"]).all() for st in rec.stages)
    ratios = [R.check_stage_fwd(st, fmt) for st in rec.stages]
    print(f"\n{shape} {fmt}: worst forward err/bound per stage (x, then y): " + " ".join(f"{v:.3f}" for v in ratios))
    assert max(ratios) <= 1.0, ratios


@pytest.mark.parametrize("shape,fmt", CASES, ids=IDS)
def test_every_convolution_backward(shape, fmt):
    rec = _run(shape, fmt)["rec"]
    assert all(st["gz"] is not None and st["gx"] is not None for st in rec.stages[:13])
    assert all(st["gz"] is None and st["gx"] is None for st in rec.stages[13:])         # y: no gradient anywhere
    ratios = [R.check_stage_bwd(st, fmt, k == 0) for k, st in enumerate(rec.stages[:13])]
    print(f"\n{shape} {fmt}: worst backward err/bound per stage (the first: image gradient): "
          + " ".join(f"{v:.3f}" for v in ratios))
    assert max(ratios) <= 1.0, ratios


@pytest.mark.parametrize("shape,fmt", CASES, ids=IDS)
def test_max_pools_are_exact(shape, fmt):
    rec = _run(shape, fmt)["rec"]
    assert tuple(rec.stages[0]["x"].shape) == shape and tuple(rec.stages[13]["x"].shape) == shape
    assert tuple(rec.stages[12]["x"].shape[2:]) == (shape[2] // 16, shape[3] // 16)
    assert R.check_pools(rec.stages) == 0


@pytest.mark.parametrize("shape,fmt", CASES, ids=IDS)
def test_loss_assembly(shape, fmt):
    run = _run(shape, fmt)
    ls = run["rec"].loss
    assert [float(w) for w in ls["w"]] == list(R.WEIGHTS)
    for i, k in enumerate(R.SLICE_END):          # the loss reads relu{1..5}_1 of x and of y
        assert torch.equal(ls["a"][i], run["rec"].stages[k]["z"]) and torch.equal(ls["b"][i], run["rec"].stages[13 + k]["z"])
    ref, bnd = R.loss_reference(ls["a"], ls["b"])
    print(f"\n{shape} {fmt}: loss {ls['value']!r}, fp64 of the recorded features {ref!r}, bound {bnd:.3e}, "
          f"err/bound {R.check_loss_value(ls):.4f}")
    assert R.check_loss_value(ls) <= 1.0
    assert all(g is None for g in ls["gb"])
    assert R.check_loss_grads(ls, fmt) == 0


@pytest.mark.parametrize("shape,fmt", CASES, ids=IDS)
def test_end_to_end_inequality(shape, fmt):
    run = _run(shape, fmt)
    lhs, rhs = R.end_to_end(run["rec"].loss, run["ref"])
    print(f"\n{shape} {fmt}: |loss - loss_fp64| = {lhs:.3e} <= {rhs:.3e} (fp64 loss {run['ref']['loss']:.6f})")
    assert lhs <= rhs


@pytest.mark.parametrize("shape,fmt", CASES, ids=IDS)
def test_drift_stays_at_the_emulations_noise_level(shape, fmt):
    run = _run(shape, fmt)
    feats, grad = R.drift(run["rec"].loss["a"], run["grad"], run["ref"])
    nf, ng = run["noise"]
    print(f"\n{shape} {fmt}: per-slice relative L2 against fp64, device " + " ".join(f"{v:.3e}" for v in feats)
          + " | emulation " + " ".join(f"{v:.3e}" for v in nf))
    print(f"{shape} {fmt}: image gradient relative L2 against fp64, device {grad:.4f} | emulation {ng:.4f}")
    assert torch.isfinite(run["grad"]).all()
    for d, n in zip(feats, nf):
        assert d <= R.DRIFT_FACTOR * n, (feats, nf)
    assert grad <= R.DRIFT_FACTOR * ng, (grad, ng)
