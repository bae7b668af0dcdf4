"""Deterministic stand-ins shared by tests/golden/make_window_goldens.py (which runs beside the REFERENCE in
the authoring container) and the GPU parity tests (which run beside the HIP build) -- TEST INFRASTRUCTURE.

They replace the two pieces of the training window whose reference code cannot be executed offline:

* ``stub_flow_and_conf``  stands in for ``FlowNet.forward`` (models/flownet.py:20-37): the pretrained
  FlowNet2 checkpoint is a download and FlowNetC needs the CUDA correlation extension.  Any fixed function
  of the two frame stacks serves to pin the HARNESS (what is fed where, which tensors are detached, how the
  losses are weighted); this one is cheap, smooth and data dependent.
* ``stub_flownetc``       stands in for ``FlowNetC.forward`` inside the FlowNet2 composition
  (models/flownet2_pytorch/models.py:104): same reason.

Plain torch, device agnostic, no randomness.
"""
import math

import torch
import torch.nn.functional as F


def smooth(shape, seed, blur=7, gain=3.0):
    """Seeded smooth field in (-1, 1) (Gaussian noise, box blur, tanh) -- same recipe as make_net_goldens."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    lead = x.shape[:-3]
    x = x.reshape((-1,) + tuple(x.shape[-3:]))
    p = blur // 2
    x = F.avg_pool2d(F.pad(x, (p, p, p, p), mode="reflect"), blur, stride=1)
    return torch.tanh(x * gain).reshape(lead + tuple(x.shape[-3:]))


def _flow_conf_4d(im1, im2):
    d = im1 - im2
    flow = 6.0 * F.avg_pool2d(F.pad(d[:, 0:2], (2, 2, 2, 2), mode="replicate"), 5, stride=1)
    conf = ((d * d).sum(1, keepdim=True) < 0.35).float()
    return flow, conf


def stub_flow_and_conf(input_A, input_B):
    """[B,n,3,H,W] or [N,3,H,W] frame stacks -> (flow [..,2,H,W], conf [..,1,H,W]), fp32, no grad."""
    with torch.no_grad():
        if input_A.dim() == 5:
            b, n, c, h, w = input_A.shape
            flow, conf = _flow_conf_4d(input_A.reshape(-1, c, h, w).float(), input_B.reshape(-1, c, h, w).float())
            return flow.view(b, n, 2, h, w), conf.view(b, n, 1, h, w)
        return _flow_conf_4d(input_A.float(), input_B.float())


def stub_flownetc(x):
    """[N,6,H,W] (two mean-subtracted images) -> 'flow2' [N,2,H/4,W/4]."""
    return 0.05 * F.avg_pool2d(x[:, 0:2] - x[:, 3:5], 4)


def moving_pair(n, h, w):
    """Closed-form, RNG-free frame pairs for the FlowNetC / FlowNet2 goldens: -> (im1, im2) [n,3,h,w] float64 holding
    float32 values in (-1, 1).  Each sample and channel is its own sum of five sinusoids (periods 15 to 80 pixels); im2
    is im1 moved by a sub-pixel displacement of its own per sample, so the cost volume peaks away from zero
    displacement.  A contrast envelope moves with the content, and every sample and channel has a brightness offset of its
    own (so a mean taken over the wrong axes shows).  Written in pixel units: the same function at any size."""
    ys = torch.arange(h, dtype=torch.float64).view(h, 1)
    xs = torch.arange(w, dtype=torch.float64).view(1, w)

    def image(k, dx, dy):
        # contrast envelope (0.15 .. 1, moving with the content): low-contrast patches are where the confidence mask is 1
        env = 0.575 + 0.425 * torch.sin(2 * math.pi * (xs + dx) / 57 + 0.9 * k) * torch.cos(2 * math.pi * (ys + dy) / 47 + 0.4 * k)
        chans = []
        for c in range(3):
            s = torch.zeros(h, w, dtype=torch.float64)
            for t in range(5):
                j = 3 * k + 5 * c + 7 * t
                fx = (1.0 / 80 + (j % 9) / 160.0) * (1 if t % 2 else -1)
                fy = 1.0 / 72 + ((j * 5) % 11) / 200.0
                s = s + torch.sin(2 * math.pi * (fx * (xs + dx) + fy * (ys + dy)) + 0.7 * k + 1.3 * c + 2.1 * t) / math.sqrt(t + 1)
            chans.append(0.7 * torch.tanh(0.9 * s) * env + 0.25 * math.sin(1.9 * k + 2.3 * c + 0.5))
        return torch.stack(chans)

    im1 = torch.stack([image(k, 0.0, 0.0) for k in range(n)])
    im2 = torch.stack([image(k, 3.25 + 0.5 * k, -1.5 + 0.75 * k) for k in range(n)])
    return im1.float().double(), im2.float().double()


def pair_checksum(im1, im2):
    """float64 sum and eight sampled values of a pair (what a golden stores instead of the inputs)."""
    a, b = im1.double().flatten(), im2.double().flatten()
    idx = torch.linspace(0, a.numel() - 1, 8).long()
    return torch.stack([a.sum(), b.sum()]).numpy(), torch.cat([a[idx], b[idx]]).numpy()


FLOWNETC_TOWER_GAIN = 5.0


def gain_flownetc(m, gain=FLOWNETC_TOWER_GAIN):
    """FlowNetC's feature tower (conv1..conv3) weights x``gain``, applied after the bias taming on both sides of the
    FlowNetC / FlowNet2 goldens.  With the tamed random init the tower's features are ~0.04 and the cost volume (a mean of
    their products) ~6e-4, 3 % of what conv_redir feeds conv3_1: no golden could see how the cost volume is wired.  At x5
    the two paths are comparable (a trained tower's features are O(1) too)."""
    with torch.no_grad():
        for c in (m.conv1, m.conv2, m.conv3):
            c[0].weight.mul_(gain)
    return m
