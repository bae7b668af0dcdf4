"""GPU parity of the VGG19 perceptual loss (ir2rgb_amd/vgg.py) against the same architecture and
the same randomly initialised weights evaluated by plain torch in fp32 (the pretrained torchvision weights are
not available offline, so the loss value itself is unpinned by any reference fixture; the module tree / key names
are the reference's, models/networks.py:721-752).  tests/test_vgg_fp64_gpu.py holds the module to fp64 stage by stage;
here also: the down-sampling branch of VGGLoss.forward, and how the trainer wires the term into G."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _torch_features(vgg, x):
    outs, h = [], x
    for s in range(1, 6):
        h = getattr(vgg, f"slice{s}")(h)
        outs.append(h)
    return outs


def test_vgg_state_dict_keys_follow_torchvision_indices():
    from ir2rgb_amd.vgg import Vgg19
    keys = set(Vgg19().state_dict().keys())
    conv_idx = [0, 2, 5, 7, 10, 12, 14, 16, 19, 21, 23, 25, 28]                    # torchvision vgg19.features conv layers < 30
    slice_of = lambda i: 1 if i < 2 else 2 if i < 7 else 3 if i < 12 else 4 if i < 21 else 5   # noqa: E731
    assert keys == {f"slice{slice_of(i)}.{i}.{p}" for i in conv_idx for p in ("weight", "bias")}
    assert not any(p.requires_grad for p in Vgg19().parameters())                  # requires_grad=False default


@pytest.mark.parametrize("dtype,tol", [(torch.float16, 2e-2), (torch.bfloat16, 6e-2)])
def test_vgg_loss_and_input_gradient_match_torch(dtype, tol):
    from ir2rgb_amd.vgg import VGGLoss, Vgg19
    dev = torch.device("cuda:0")
    torch.manual_seed(3)
    vgg = Vgg19().to(dev)
    vgg.compute_dtype = dtype
    g = torch.Generator().manual_seed(5)
    x = torch.tanh(torch.randn(1, 3, 64, 96, generator=g)).to(dev).requires_grad_()
    y = torch.tanh(torch.randn(1, 3, 64, 96, generator=g)).to(dev)
    loss = VGGLoss(vgg)(x, y)
    fx, fy = _torch_features(vgg, x), _torch_features(vgg, y)
    ws = [1.0 / 32, 1.0 / 16, 1.0 / 8, 1.0 / 4, 1.0]
    ref = sum(w * F.l1_loss(a, b.detach()) for a, b, w in zip(fx, fy, ws))
    assert abs(loss.item() - ref.item()) <= tol * abs(ref.item()), (loss.item(), ref.item())
    # the loss gradient flows (value checked above; its sign(a-b) factor flips under half rounding wherever two
    # random-weight features nearly coincide, so the backward CHAIN is compared on a linear functional instead)
    loss.backward()
    assert torch.isfinite(x.grad).all() and x.grad.abs().sum().item() > 0
    x.grad = None
    probes = [torch.randn(f.shape, generator=g).to(dev) for f in fx]
    mine = vgg(x)
    sum((a.float() * r).sum() * w for a, r, w in zip(mine, probes, ws)).backward()
    gx = x.grad.clone()
    x.grad = None
    sum((a * r).sum() * w for a, r, w in zip(fx, probes, ws)).backward()
    rel = ((gx - x.grad).norm() / x.grad.norm()).item()
    assert rel <= 4 * tol, rel     # 13 half-precision layers, ReLU masks and four max-pool selections deep
    for i in range(5):
        assert ((mine[i].float() - fx[i]).norm() / fx[i].norm()).item() <= tol * (1 + i) / 2, i


def test_training_window_with_vgg_loss_runs():
    """The loop body with the perceptual term switched on (random VGG weights): finite losses, the term is positive
    and reaches the generator's parameters."""
    from ir2rgb_amd import vid2vid as V
    dev = torch.device("cuda:0")
    A, B = V.synthetic_sequence(4, 64, 128, 7, dev)
    tr = V.Vid2VidTrainer(dev, seed=0, first_layer_gen_filters=64, gen_blocks=2, no_vgg=False)
    base = V.Vid2VidTrainer(dev, seed=0, first_layer_gen_filters=64, gen_blocks=2)
    out, ref = tr.train_window(A[:, :3], B[:, :3]), base.train_window(A[:, :3], B[:, :3])
    assert all(torch.isfinite(v) for v in out.values())
    assert out["G"].item() > ref["G"].item()      # same window, same weights: the extra term is positive
    assert abs(out["D"].item() - ref["D"].item()) <= 1e-5 * abs(ref["D"].item())
    # G is the other terms' fp32 sum + G_VGG (one more fp32 addition: half an ulp of G); the other terms are those of the
    # run without the perceptual loss, reproduced to the 1e-5 the line above grants D
    g, g0, gv = out["G"].item(), ref["G"].item(), out["G_VGG"].item()
    print(f"\nG {g!r} - G without VGG {g0!r} = {g - g0!r}; G_VGG {gv!r}")
    assert gv > 0 and ref["G_VGG"].item() == 0
    assert abs((g - g0) - gv) <= 2.0 ** -24 * abs(g) + 1e-5 * abs(g0)
    # G_VGG is lambda_feat * (VGGLoss(fake_B, real_B) + VGGLoss(fake_B_raw, real_B)) of the window's own frames
    # (trainer.last_outputs / last_inputs), recomputed by the trainer's module: the same launches on the same operands,
    # then one fp32 addition and one product
    fake_B, fake_B_raw = tr.last_outputs[:2]
    real_B = tr.last_inputs[1]
    flat = lambda t: t.reshape((-1,) + tuple(t.shape[2:]))  # noqa: E731
    with torch.no_grad():
        want = (tr.vgg_loss(flat(fake_B), flat(real_B)) + tr.vgg_loss(flat(fake_B_raw), flat(real_B))) * tr.opt["lambda_feat"]
    print(f"G_VGG recomputed from the window's frames {want.item()!r}")
    assert abs(gv - want.item()) <= 2.0 ** -22 * abs(want.item())


# (shape, times the width is halved before the network sees it)
DOWNSAMPLED = [((1, 3, 32, 1026), 1), ((1, 3, 64, 2050), 2), ((1, 3, 16, 1024), 0)]


def _avg_pool_adjoint(g, size):
    """Adjoint of F.avg_pool2d(., 2, 2) on an input of ``size`` (H, W): a quarter of g to each pixel of its 2 x 2 cell,
    zero to a row / column the floor leaves out (exact: a power of two)."""
    out = torch.zeros(g.shape[:2] + tuple(size), dtype=g.dtype)
    q = (g / 4).repeat_interleave(2, 2).repeat_interleave(2, 3)
    out[:, :, :q.shape[2], :q.shape[3]] = q
    return out


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("shape,halvings", DOWNSAMPLED, ids=[f"w{s[3]}" for s, _ in DOWNSAMPLED])
def test_vgg_loss_downsamples_wide_inputs(shape, halvings, fmt):
    """VGGLoss.forward's ``while x.size(3) > 1024`` branch (models/loss.py:52-53): the loss of a wide pair is the loss of
    the explicitly average-pooled pair bit for bit, x.grad the pooling's adjoint of that call's input gradient bit for
    bit, and at 1024 nothing is pooled.  The once-halved case also meets the end-to-end inequality of
    tests/test_vgg_fp64_gpu.py against the fp64 chain of the pooled images."""
    from ir2rgb_amd.vgg import VGGLoss, Vgg19
    from oracle import vgg_ref as R
    dev = torch.device("cuda:0")
    cpu = R.init_weights(Vgg19())
    vgg = Vgg19().to(dev)
    vgg.load_state_dict(cpu.state_dict())
    vgg.compute_dtype = R.FORMATS[fmt]
    x, y = R.images(shape, seed=7)
    xd, yd = x.to(dev).requires_grad_(), y.to(dev)
    rec, grad = R.device_record(VGGLoss(vgg), xd, yd, fmt)
    assert rec.stages[0]["x"].shape[3] == rec.stages[13]["x"].shape[3] == shape[3] >> halvings <= 1024
    xp, yp, sizes = xd.detach(), yd, []
    for _ in range(halvings):
        sizes.append(tuple(xp.shape[2:]))
        xp, yp = F.avg_pool2d(xp, 2, 2, count_include_pad=False), F.avg_pool2d(yp, 2, 2, count_include_pad=False)
    assert torch.equal(rec.stages[0]["x"], xp.cpu()) and torch.equal(rec.stages[13]["x"], yp.cpu())
    xp = xp.clone().requires_grad_()
    rec2, grad2 = R.device_record(VGGLoss(vgg), xp, yp, fmt)
    print(f"\n{shape} {fmt}: loss {rec.loss['value']!r}, of the pooled pair {rec2.loss['value']!r}")
    assert rec.loss["value"] == rec2.loss["value"]
    for size in reversed(sizes):
        grad2 = _avg_pool_adjoint(grad2, size)
    assert grad2.abs().sum() > 0 and torch.equal(grad, grad2)
    if halvings == 1:
        ref = R.reference64(cpu, xp.detach().cpu(), yp.cpu(), R.FORMATS[fmt])
        lhs, rhs = R.end_to_end(rec.loss, ref)
        print(f"{shape} {fmt}: |loss - loss_fp64| = {lhs:.3e} <= {rhs:.3e} (fp64 loss {ref['loss']:.6f})")
        assert lhs <= rhs
