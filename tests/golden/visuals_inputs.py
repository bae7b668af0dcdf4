"""Inputs of tests/test_visuals_gpu.py, built on the CPU from fixed seeds so that tests/test_visuals_cpu.py can hold them
to the conditions the GPU comparison rests on (no GPU, no kernel library needed here).

Shapes come from the branches of csrc/visuals.hip, not from the workload: (1, 1); (3, 5) scalar; (4, 8) vector;
(5, 12) vector with an odd height; (17, 260) several workgroups and several (min, max) rows per panel.  Panel sets: the
nine of a training run, seven (no generator flow), and a one-channel input.
"""
import numpy as np
import torch

SHAPES = [(1, 1), (3, 5), (4, 8), (5, 12), (17, 260)]
PANEL_SETS = {"nine": (3, True), "seven": (3, False), "one_channel_input": (1, True)}     # name -> (input_nc, with_flow)
CASES = [(h, w, s) for (h, w) in SHAPES for s in PANEL_SETS]
FLOW_KEYS = ("flow_ref", "flow")


def case_seed(h, w, panel_set):
    # (the constant: chosen on the CPU so that every flow panel meets tests/test_visuals_cpu.py::test_flow_inputs_are_decided)
    return 2 * 7919 + 1000 * h + 10 * w + sorted(PANEL_SETS).index(panel_set)


def boundary_values():
    """Every k/255 and 2k/255 - 1 (k = 0..255) with its fp32 neighbours below and above: where truncation and rounding,
    and one rounding of the arithmetic more or less, part."""
    k = np.arange(256, dtype=np.float64)
    vals = []
    for base in (k / 255.0, 2.0 * k / 255.0 - 1.0):
        b = base.astype(np.float32)
        vals += [b, np.nextafter(b, np.float32(-4)), np.nextafter(b, np.float32(4))]
    return torch.from_numpy(np.concatenate(vals).astype(np.float32))


def plant(frame, values):
    """Writes ``values`` over the first elements of ``frame`` (as many as fit)."""
    flat = frame.reshape(-1)          # (a view: frames are contiguous slices)
    n = min(flat.numel(), values.numel())
    flat[:n] = values[:n]


def case_tensors(h, w, panel_set):
    """The tensors a trainer holds after a window, [1, 2, C, H, W] (``fake_B_first`` [3, H, W]), on the CPU.  Image
    tensors: N(0, 0.8) (a fifth of the values outside [-1, 1]), with NaN, +inf, -inf planted in ``fake_B`` and the
    boundary values in ``real_B`` (IMAGE_NORM), ``conf_ref`` and ``real_A`` (IMAGE_UNIT); flows: N(0, 3) per component."""
    input_nc, with_flow = PANEL_SETS[panel_set]
    g = torch.Generator().manual_seed(case_seed(h, w, panel_set))
    r = lambda *s: torch.randn(s, generator=g) * 0.8  # noqa: E731
    t = dict(real_A=r(1, 2, input_nc, h, w), fake_B=r(1, 2, 3, h, w), fake_B_first=r(3, h, w), fake_B_raw=r(1, 2, 3, h, w),
             real_B=r(1, 2, 3, h, w), flow_ref=torch.randn((1, 2, 2, h, w), generator=g) * 3,
             conf_ref=torch.rand((1, 2, 1, h, w), generator=g), flow=None, weight=None)
    if with_flow:
        t["flow"] = torch.randn((1, 2, 2, h, w), generator=g) * 3
        t["weight"] = torch.rand((1, 2, 1, h, w), generator=g)
    plant(t["fake_B"][0, -1], torch.tensor([float("nan"), float("inf"), -float("inf")]))
    b = boundary_values()
    plant(t["real_B"][0, -1], b)
    plant(t["conf_ref"][0, -1], b)
    plant(t["real_A"][0, -1], torch.cat([torch.tensor([float("nan"), float("inf"), -float("inf")]), b]))
    return t


def random_flow_panels():
    """[(case id, key, fp32 [2, H, W])]: every random flow panel the GPU tests convert."""
    out = []
    for h, w, s in CASES:
        t = case_tensors(h, w, s)
        out += [(f"{h}x{w}-{s}", k, t[k][0, -1]) for k in FLOW_KEYS if t[k] is not None]
    return out
