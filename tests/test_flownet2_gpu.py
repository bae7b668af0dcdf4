"""GPU parity of the MFMA FlowNet2 engine (ir2rgb_amd/flownet2_hip.py) against the same parameter
tree evaluated with torch fp32 convolutions (the module's own nn.Conv2d stacks + the hand-written
ops).  Seeded reference init (xavier weights, uniform biases; no checkpoint offline).

Sub-networks are compared one by one on identical inputs: relative L2 <= 1e-2 (bf16 operands over
~20 layers; measured 2.6e-3 .. 4.6e-3); the composed FlowNet2 output: <= 2e-2 (measured 3.5e-3)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12)).item()


@pytest.fixture(scope="module")
def net(dev):
    from ir2rgb_amd.flownet2_pytorch.models import FlowNet2
    torch.manual_seed(3)
    m = FlowNet2(conv_dtype=torch.bfloat16).to(dev).eval()
    # the reference init (uniform(0,1) biases) blows activations up layer by layer; tame it so that
    # fp32-vs-bf16 comparisons stay in range, as a trained checkpoint would
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 1:
                p.mul_(0.05)
    return m


@pytest.mark.parametrize("name,cin", [("flownetc", 6), ("flownets_1", 12), ("flownets_d", 6), ("flownetfusion", 11)])
def test_subnetwork_vs_torch_convs(dev, net, name, cin):
    from ir2rgb_amd import flownet2_hip as FH
    sub = getattr(net, name)
    g = torch.Generator().manual_seed(cin)
    x = (torch.randn(1, cin, 128, 192, generator=g) * 0.5).to(dev)
    with torch.no_grad():
        ref = sub(x)
        ref = ref[0] if isinstance(ref, tuple) else ref
        run = {"flownetc": FH.flownetc, "flownets_1": FH.flownets, "flownets_d": FH.flownetsd, "flownetfusion": FH.flownetfusion}[name]
        got = run(sub, x, torch.bfloat16)
    assert got.shape == ref.shape and got.dtype == torch.float32
    err = _rel(got, ref)
    print(name, "relative L2", err)
    assert err <= 1e-2, err


@pytest.mark.parametrize("name,cin", [("flownetc", 6), ("flownets_1", 12), ("flownets_d", 6), ("flownetfusion", 11)])
def test_subnetwork_pools_under_alternating_shapes(dev, net, name, cin):
    """One module called at [1, cin, 128, 192], then [2, cin, 128, 192], then the first input again: each call draws its
    buffers from the pool of its own (shape, dtype, device), so the third result is the first one bit for bit and no pool
    grows after its first use."""
    from ir2rgb_amd import flownet2_hip as FH
    sub = getattr(net, name)
    run = {"flownetc": FH.flownetc, "flownets_1": FH.flownets, "flownets_d": FH.flownetsd, "flownetfusion": FH.flownetfusion}[name]
    g = torch.Generator().manual_seed(cin)
    x1 = (torch.randn(1, cin, 128, 192, generator=g) * 0.5).to(dev)
    x2 = (torch.randn(2, cin, 128, 192, generator=g) * 0.5).to(dev)
    outs, first_use = [], {}
    with torch.no_grad():
        for x in (x1, x2, x1):
            outs.append(run(sub, x, torch.bfloat16))
            for key, pool in sub._ir2rgb_workspaces.items():
                first_use.setdefault(key, len(pool))
    assert outs[0].shape[0] == 1 and outs[1].shape[0] == 2 and torch.isfinite(outs[1]).all()
    assert torch.equal(outs[2], outs[0])
    keys = {(tuple(x.shape), torch.bfloat16, x.device) for x in (x1, x2)}
    assert keys <= set(first_use) and all(first_use[k] > 0 for k in keys)
    assert {key: len(pool) for key, pool in sub._ir2rgb_workspaces.items()} == first_use


def test_flownet2_composed(dev, net):
    g = torch.Generator().manual_seed(8)
    base = torch.rand(1, 3, 128 + 8, 192 + 8, generator=g)
    im1, im2 = base[:, :, 4:-4, 4:-4], base[:, :, 2:-6, 5:-3]
    x = torch.stack([im1, im2], 2).to(dev)
    with torch.no_grad():
        net.use_hip_convs = True
        a = net(x)
        net.use_hip_convs = False
        net.conv_dtype = torch.float32
        b = net(x)
        net.use_hip_convs, net.conv_dtype = True, torch.bfloat16
    assert a.shape == (1, 2, 128, 192)
    err = _rel(a, b)
    print("FlowNet2 relative L2", err)
    assert err <= 2e-2, err


def test_flownet_graph_replay_equals_eager():
    """FlowNet2 + confidence captured into a HIP graph (third call at a shape) must return exactly what the
    eager path returns, on new inputs, and must not alias its outputs across calls."""
    import torch
    from ir2rgb_amd import vid2vid as V
    dev = torch.device("cuda:0")
    net = V.FlowNet(use_graph=True).to(dev)
    ref = V.FlowNet(use_graph=False).to(dev)
    ref.load_state_dict(net.state_dict())
    g = torch.Generator().manual_seed(4)
    outs = []
    for i in range(5):
        a = torch.tanh(torch.randn(2, 3, 128, 192, generator=g)).to(dev)
        b = torch.tanh(torch.randn(2, 3, 128, 192, generator=g)).to(dev)
        f1, c1 = net(a, b)
        f0, c0 = ref(a, b)
        assert torch.equal(f1, f0) and torch.equal(c1, c0), f"call {i}"
        outs.append((f1, f0.clone()))
    assert isinstance(net._graphs[((2, 3, 128, 192), torch.float32, "cuda:0")], tuple), "the graph path was not taken"
    for f1, f0 in outs:                      # earlier results were not overwritten by later replays
        assert torch.equal(f1, f0)
