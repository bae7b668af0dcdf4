"""GPU parity of FlowNetC and of the unstubbed FlowNet2 against float64 goldens made by the
reference's own ``FlowNetC`` and ``FlowNet2.forward`` (tests/golden/make_window_goldens.py ``flownetc``: the three CUDA
operators replaced by oracle/closed_form.py, pinned by tests/test_oracle_ops.py).

Inputs are not stored: tests/golden/window_stub.py:moving_pair rebuilds them from a closed form, and the golden's
checksum is asserted.  Weights are not stored: the same seed gives bit-identical parameters (asserted by the script).

Bounds (relative L2 unless said otherwise), the existing a12 bounds of tests/test_harness_gpu.py:
  FlowNetC, every decoder level flow6 .. flow2     1e-2 (MFMA path, bf16 and f16; the fp32-operator fallback too)
  FlowNetC, the project's torch path in fp32       1e-3
  FlowNet2 + confidence mask                       flow 2e-2; at most 2 % of the mask on the other side of the threshold
Each golden carries the rounding floor of FlowNetC's flow2: the float64 reference with every convolution output and the
cost volume rounded to bf16 / f16.  tests/test_flownetc_cpu.py asserts the floors are at most half the bound.
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from window_stub import gain_flownetc, moving_pair, pair_checksum  # noqa: E402

FLOWNETC = {"a": "flownetc_a_n1_64x128", "b": "flownetc_b_n2_128x192", "c": "flownetc_c_n1_512x1024"}
FLOWNET2 = {"a": "flownet2_a_n1_64x128", "b": "flownet2_b_n1_80x128", "c": "flownet2_c_n3_128x192", "d": "flownet2_d_n1_512x1024"}
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
C_TOL, C_TORCH_TOL, F2_TOL, CONF_TOL = 1e-2, 1e-3, 2e-2, 0.02


def rel_l2(a, ref):
    a = a.detach().double().cpu()
    ref = torch.from_numpy(np.asarray(ref)).double()
    assert tuple(a.shape) == tuple(ref.shape), (tuple(a.shape), tuple(ref.shape))
    return ((a - ref).norm() / ref.norm().clamp_min(1e-30)).item()


def load(golden_dir, name):
    """The golden and its rebuilt input pair (float64 holding float32 values; checksum asserted)."""
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    im1, im2 = moving_pair(int(g["n"]), int(g["h"]), int(g["w"]))
    sums, samples = pair_checksum(im1, im2)
    np.testing.assert_allclose(sums, g["in_sums"], rtol=0, atol=1e-5)
    np.testing.assert_allclose(samples, g["in_samples"], rtol=0, atol=1e-6)
    return g, im1, im2


def _tame(m):
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 1:
                p.mul_(0.05)
    return m


@pytest.fixture(scope="module")
def flownetc_net(dev, golden_dir):
    from ir2rgb_amd.flownet2_pytorch import models as M
    torch.manual_seed(int(np.load(os.path.join(golden_dir, FLOWNETC["a"] + ".npz"))["seed"]))
    return gain_flownetc(_tame(M.FlowNetC())).to(dev).eval()


def _run_flownetc(net, x, dtype, monkeypatch):
    """flownet2_hip.flownetc -> [flow2, flow3, flow4, flow5, flow6] (levels 6..3 captured from ``predict`` in call order)."""
    from ir2rgb_amd import flownet2_hip as FH
    seen = []
    orig = FH.predict

    def spy(*a, **k):
        out = orig(*a, **k)
        seen.append(out.clone())
        return out

    monkeypatch.setattr(FH, "predict", spy)
    with torch.no_grad():
        flow2 = FH.flownetc(net, x, dtype)
    monkeypatch.setattr(FH, "predict", orig)
    assert len(seen) == 5 and torch.equal(seen[-1], flow2)
    return [flow2] + seen[3::-1]


def _check_flownetc(g, flows, tol, what):
    errs = {f"flow{lvl}": rel_l2(f, g[f"flow{lvl}"]) for lvl, f in zip((2, 3, 4, 5, 6), flows)}
    print(what, {k: f"{v:.2e}" for k, v in errs.items()}, "floor bf16 %.2e f16 %.2e" % (float(g["floor_bf16"]), float(g["floor_f16"])))
    assert all(v <= tol for v in errs.values()), (what, errs)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_flownetc_vs_reference_golden(dev, golden_dir, flownetc_net, monkeypatch, case, dt):
    """The MFMA engine's FlowNetC (banded MFMA cost volume): all five decoder levels.  The cost volume's LeakyReLU is an
    identity at these weights (tests/test_flownetc_cpu.py), so its slope is checked where it is handed to the kernel."""
    from ir2rgb_amd import flownet2_hip as FH
    g, im1, im2 = load(golden_dir, FLOWNETC[case])
    x = torch.cat([im1, im2], 1).float().to(dev)
    calls = []
    orig = FH.corr_nhwc

    def corr_spy(mod, av, bv, yv, slope):
        ran = orig(mod, av, bv, yv, slope)
        calls.append((ran, yv.off, yv.ch, slope))
        return ran

    monkeypatch.setattr(FH, "corr_nhwc", corr_spy)
    flows = _run_flownetc(flownetc_net, x, DTYPES[dt], monkeypatch)
    assert calls == [(True, 32, 441, 0.1)]
    _check_flownetc(g, flows, C_TOL, f"FlowNetC {case} {dt} (MFMA cost volume)")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("case", ["a", "b"])
def test_flownetc_fp32_correlation_branch_vs_reference_golden(dev, golden_dir, flownetc_net, monkeypatch, case, dt):
    """IR2RGB_CORR_MFMA=0 (read per call): the fp32 correlation operator, then put_nchw with the LeakyReLU."""
    from ir2rgb_amd import flownet2_hip as FH
    g, im1, im2 = load(golden_dir, FLOWNETC[case])
    x = torch.cat([im1, im2], 1).float().to(dev)
    monkeypatch.setenv("IR2RGB_CORR_MFMA", "0")
    used = []
    orig = FH.put_nchw

    def put_spy(x_nchw, yv, act=0):
        used.append((yv.off, yv.ch, act))
        return orig(x_nchw, yv, act)

    monkeypatch.setattr(FH, "put_nchw", put_spy)
    flows = _run_flownetc(flownetc_net, x, DTYPES[dt], monkeypatch)
    assert used == [(32, 441, FH.LEAKY01)]
    _check_flownetc(g, flows, C_TOL, f"FlowNetC {case} {dt} (fp32 correlation operator)")


def test_flownetc_torch_path_vs_reference_golden(dev, golden_dir, flownetc_net):
    """FlowNetC.forward in fp32 torch convolutions (FlowNet2.use_hip_convs=False, conv_dtype=float32): the module
    tests/test_flownet2_gpu.py holds the MFMA engine to."""
    g, im1, im2 = load(golden_dir, FLOWNETC["a"])
    with torch.no_grad():
        flow2 = flownetc_net(torch.cat([im1, im2], 1).float().to(dev))
    err = rel_l2(flow2, g["flow2"])
    print("FlowNetC a torch fp32 flow2 relative L2 %.2e (bound %.0e)" % (err, C_TORCH_TOL))
    assert err <= C_TORCH_TOL


@pytest.fixture(scope="module")
def flownet2_nets(dev, golden_dir):
    from ir2rgb_amd import vid2vid as V
    seed = int(np.load(os.path.join(golden_dir, FLOWNET2["a"] + ".npz"))["seed"])
    nets = {}
    for dt, dtype in DTYPES.items():
        fn = V.FlowNet(conv_dtype=dtype, seed=seed, use_graph=False)
        gain_flownetc(_tame(fn.flowNet).flownetc)
        nets[dt] = fn.to(dev)
    return nets


def _check_flownet2(g, flow, conf, what):
    if "flow_pool4" in g.files:
        err = rel_l2(F.avg_pool2d(flow, 4), g["flow_pool4"])
        bits = np.unpackbits(g["conf_bits"])[:conf.numel()]
        ref_conf = torch.from_numpy(bits.astype(np.float32)).view(conf.shape)
    else:
        err = rel_l2(flow, g["flow"])
        ref_conf = torch.from_numpy(g["conf"])
    mism = ((conf.float().cpu() - ref_conf).abs() > 0.5).float().mean().item()
    print(what, "flow relative L2 %.2e (bound %.0e)" % (err, F2_TOL), "confidence mismatch %.4f (bound %.2f)" % (mism, CONF_TOL),
          "reference confidence mean %.4f" % ref_conf.mean().item())
    assert err <= F2_TOL and mism <= CONF_TOL, (what, err, mism)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("case", ["a", "b", "c", "d"])
def test_flownet2_unstubbed_vs_reference_golden(dev, golden_dir, flownet2_nets, case, dt):
    """vid2vid.FlowNet (FlowNet2 with its FlowNetC, then the confidence mask) against the reference's own FlowNet2.forward
    and flownet.py:38-57.  b: the 80 -> 64 row resize; c: three distinct pairs (rgb_mean is per sample); d: the bench size."""
    g, im1, im2 = load(golden_dir, FLOWNET2[case])
    fn = flownet2_nets[dt]
    flow, conf = fn.compute_flow_and_conf(im1.float().to(dev), im2.float().to(dev))
    assert flow.shape == (im1.shape[0], 2) + tuple(im1.shape[2:]) and conf.shape == (im1.shape[0], 1) + tuple(im1.shape[2:])
    _check_flownet2(g, flow, conf, f"FlowNet2 {case} {dt}")


def test_flownet2_graph_replay_vs_reference_golden(dev, golden_dir):
    """Case c through the captured graph: the third call at a shape is the first replay, what the training window runs."""
    from ir2rgb_amd import vid2vid as V
    g, im1, im2 = load(golden_dir, FLOWNET2["c"])
    fn = V.FlowNet(conv_dtype=torch.bfloat16, seed=int(g["seed"]), use_graph=True)
    gain_flownetc(_tame(fn.flowNet).flownetc)
    fn = fn.to(dev)
    a, b = im1.float().to(dev), im2.float().to(dev)
    for _ in range(3):
        flow, conf = fn.compute_flow_and_conf(a, b)
    assert isinstance(fn._graphs[(tuple(a.shape), a.dtype, str(a.device))], tuple), "no graph was captured"
    _check_flownet2(g, flow, conf, "FlowNet2 c bf16 graph replay")
