"""GPU side of the training snapshots: csrc/visuals.hip against the CPU definitions of ir2rgb_amd/visuals.py, and
``fit(..., snapshots=...)`` end to end.

Shapes and panel sets: tests/golden/visuals_inputs.py (chosen from the kernel's branches; tests/test_visuals_cpu.py holds
them to the conditions this comparison rests on).  Image and unit panels are compared bit for bit.  Flow panels: a pixel
that is *decided* (both scaled values farther than 1e-3 from an integer in fp64: no fp32 evaluation of the formulas can
land on another byte) is compared byte for byte; an undecided one has to carry the coding of one of the
(Hb +- 1 mod 180, Vb +- 1) neighbours.  Every case runs through ``_lib.launch`` into a stack between canary bands.
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
import visuals_inputs as VI  # noqa: E402
from window_stub import stub_flow_and_conf  # noqa: E402

GUARD = 32768


class GuardedStack:
    """uint8 [P,H,W,3] inside a larger allocation: ``fill`` inside, 0xA5 in the bands."""

    def __init__(self, p, h, w, dev, fill):
        n = p * h * w * 3
        self.buf = torch.full((n + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        self.buf[GUARD:GUARD + n] = fill
        self.t = self.buf[GUARD:GUARD + n].view(p, h, w, 3)
        self.n = n

    def intact(self):
        return bool((self.buf[:GUARD] == 0xA5).all() and (self.buf[GUARD + self.n:] == 0xA5).all())


def on_device(t, dev, skew=0):
    """The case's tensors on the device; ``skew``: every tensor starts that many floats into its allocation."""
    out = {}
    for k, v in t.items():
        if v is None:
            out[k] = None
            continue
        buf = torch.empty(v.numel() + skew, dtype=torch.float32, device=dev)
        buf[skew:].copy_(v.reshape(-1))
        out[k] = buf[skew:].view(v.shape)
    return out


def compose_checked(plist, dev):
    """Two launches into differently pre-filled guarded stacks -> the bytes (numpy).  Equal results mean every byte inside
    was written and the call is repeatable; the bands must be untouched."""
    from ir2rgb_amd import visuals as V
    h, w = plist[0][2].shape[-2:]
    a, b = GuardedStack(len(plist), h, w, dev, 0xA5), GuardedStack(len(plist), h, w, dev, 0x5A)
    V.compose(plist, out=a.t)
    V.compose(plist, out=b.t)
    torch.cuda.synchronize()
    assert a.intact() and b.intact(), "a canary band was written"
    ra, rb = a.t.cpu().numpy(), b.t.cpu().numpy()
    assert np.array_equal(ra, rb), "unwritten bytes, or two calls differ"
    return ra


def check_against_reference(plist_cpu, got):
    from ir2rgb_amd import visuals as V
    for k, (name, kind, x) in enumerate(plist_cpu):
        if kind == V.FLOW:
            rgb, decided, hb, vb = V.flow_to_rgb_reference(x)
            bad = (got[k] != rgb).any(-1)
            assert not (bad & decided).any(), (name, "decided pixels differ", int((bad & decided).sum()))
            for y, xx in zip(*np.nonzero(bad)):       # undecided: one of the neighbours' codings
                near = [V.hsv_bytes_to_rgb((hb[y, xx] + dh) % 180, min(max(vb[y, xx] + dv, 0), 255)).tolist()
                        for dh in (-1, 0, 1) for dv in (-1, 0, 1)]
                assert got[k][y, xx].tolist() in near, (name, int(y), int(xx), got[k][y, xx].tolist(), int(hb[y, xx]), int(vb[y, xx]))
        else:
            want = V.to_u8_reference(x, normalize=kind == V.IMAGE_NORM)
            if want.ndim == 2:
                want = np.repeat(want[:, :, None], 3, axis=2)
            assert np.array_equal(got[k], want), (name, int((got[k] != want).sum()))


@pytest.mark.parametrize("h,w,panel_set,skew", [c + (0,) for c in VI.CASES] + [(4, 8, s, 1) for s in VI.PANEL_SETS])
def test_panels_against_the_cpu_definitions(dev, h, w, panel_set, skew):
    from ir2rgb_amd import visuals as V
    input_nc, with_flow = VI.PANEL_SETS[panel_set]
    t = VI.case_tensors(h, w, panel_set)
    plist_cpu = V.panels(t, {"input_nc": input_nc})
    plist = V.panels(on_device(t, dev, skew), {"input_nc": input_nc})
    assert len(plist) == (9 if with_flow else 7) and plist[0][2].shape[0] == input_nc
    aligned16 = all(x.data_ptr() % 16 == 0 for _, _, x in plist)
    assert aligned16 == (skew == 0 and (h * w) % 4 == 0)       # which form of the kernel this case takes
    got = compose_checked(plist, dev)
    check_against_reference(plist_cpu, got)
    # the planted special values were where the comparison looked
    fake = t["fake_B"][0, -1].reshape(-1)
    assert torch.isnan(fake[0]) and got[1].reshape(-1, 3)[0, 0] == 0
    if h * w >= 3:
        assert got[1][0, 1, 0] == 255 and got[1][0, 2, 0] == 0      # +inf, -inf


def test_boundary_values_on_both_forms(dev):
    """Every k/255 and 2k/255 - 1 with its fp32 neighbours, through IMAGE_NORM and IMAGE_UNIT, one and three channels, on the
    vector (W = 8) and the scalar (W = 7) form."""
    from ir2rgb_amd import visuals as V
    b = VI.boundary_values()
    for w in (8, 7):
        n = (b.numel() + 3 * w - 1) // (3 * w) * 3 * w
        x3 = torch.cat([b, torch.zeros(n - b.numel())]).view(3, -1, w)
        x1 = x3[:1].contiguous()
        plist_cpu = [("n3", V.IMAGE_NORM, x3), ("u3", V.IMAGE_UNIT, x3)]
        got = compose_checked([(nm, k, x.to(dev)) for nm, k, x in plist_cpu], dev)
        check_against_reference(plist_cpu, got)
        assert set(np.unique(got[0])) == set(range(256)) == set(np.unique(got[1]))
        plist_cpu = [("n1", V.IMAGE_NORM, x1), ("u1", V.IMAGE_UNIT, x1)]
        got = compose_checked([(nm, k, x.to(dev)) for nm, k, x in plist_cpu], dev)
        check_against_reference(plist_cpu, got)


@pytest.mark.parametrize("w", [6, 8])
def test_flow_exact_cases(dev, w):
    from ir2rgb_amd import visuals as V
    nan = float("nan")

    def run(f):
        return compose_checked([("flow", V.FLOW, f.to(dev))], dev)[0]

    assert not run(torch.zeros(2, 3, w)).any()                                                     # zero flow
    assert not run(torch.stack([torch.full((3, w), 1.5), torch.full((3, w), -2.0)])).any()        # max == min
    u = [1.0, 0.0, -1.0, 0.0, 0.0, 1.0, 0.0, 0.0][:w]
    v = [0.0, 1.0, 0.0, -1.0, 0.0, 0.0, 1.0, 0.0][:w]
    pure = {(1.0, 0.0): [255, 0, 0], (0.0, 1.0): [128, 255, 0], (-1.0, 0.0): [0, 255, 255], (0.0, -1.0): [128, 0, 255],
            (0.0, 0.0): [0, 0, 0]}                                                                  # Hb = 0, 45, 90, 135 at V = 255
    want = [pure[(a, b)] for a, b in zip(u, v)]
    f = torch.tensor([u, v]).view(2, 1, w)
    got = run(f)
    assert got[0].tolist() == want
    assert np.array_equal(got, V.flow_to_rgb_reference(f)[0])
    want[5] = [0, 0, 0]
    f2 = f.clone()
    f2[0, 0, 5], f2[1, 0, 5] = nan, 1.0                     # a NaN vector: black, and the others' range is undisturbed
    assert run(f2)[0].tolist() == want
    f3 = f.clone()
    f3[0, 0, 5], f3[1, 0, 5] = 3.0, nan
    assert run(f3)[0].tolist() == want


def test_error_returns(dev):
    from ir2rgb_amd import _lib
    x = torch.zeros(3, 4, 8, device=dev)
    out = torch.zeros(17, 4, 8, 3, dtype=torch.uint8, device=dev)
    ws = torch.zeros(64, device=dev)

    def table(entries):
        t = (_lib.Panel * 17)()
        for q, (src, kind, ch) in zip(t, entries):
            q.src, q.kind, q.channels = src.data_ptr() if hasattr(src, "data_ptr") else src, kind, ch
        return t

    ok = [(x, _lib.PANEL_IMAGE_NORM, 3)]
    _lib.launch("ir2rgb_visuals_u8", x, table(ok), 1, 4, 8, None, out)          # the valid call, for contrast
    bad = [(table(ok), 0, None), (table(ok * 17), 17, None), (table([(x, 9, 3)]), 1, None),
           (table([(x, _lib.PANEL_FLOW, 3)]), 1, ws), (table([(x, _lib.PANEL_FLOW, 2)]), 1, None),
           (table([(x, _lib.PANEL_IMAGE_UNIT, 2)]), 1, None), (table([(0, _lib.PANEL_IMAGE_UNIT, 1)]), 1, None)]
    for tab, n, w in bad:
        with pytest.raises(ValueError, match="visuals_u8: IR2RGB_EINVAL"):
            _lib.launch("ir2rgb_visuals_u8", x, tab, n, 4, 8, w, out)
    with pytest.raises(ValueError, match="visuals_u8: IR2RGB_EALIGN"):
        _lib.launch("ir2rgb_visuals_u8", x, table([(x.data_ptr() + 2, _lib.PANEL_IMAGE_NORM, 1)]), 1, 4, 8, None, out)
    with pytest.raises(ValueError, match="visuals_workspace_bytes"):
        _lib.query("ir2rgb_visuals_workspace_bytes", 17, 4, 8)
    assert _lib.query("ir2rgb_visuals_workspace_bytes", 2, 17, 260) == 2 * 5 * 2 * 4
    assert _lib.query("ir2rgb_visuals_workspace_bytes", 0, 4, 8) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------
# fit(..., snapshots=...)
# ---------------------------------------------------------------------------------------------
def _trainer(dev):
    from ir2rgb_amd import vid2vid as V
    tr = V.Vid2VidTrainer(dev, compute_dtype=torch.bfloat16, n_scales_spatial=2, build_flow_net=False, first_layer_gen_filters=32)
    tr.flow_net = stub_flow_and_conf
    return tr


class _Sequences:
    seq_len_max = 6

    def __init__(self, dev, watch):
        from ir2rgb_amd import vid2vid as V
        self.data = [V.synthetic_sequence(6, 64, 128, 10 + i, dev) for i in range(2)]
        self.watch = watch

    def __len__(self):
        return len(self.data)

    def sequence(self, index, n_frames_total):
        self.watch.windows = 0          # a new sequence starts
        A, B = self.data[index]
        return A[:, :n_frames_total + 2], B[:, :n_frames_total + 2]


class _Watch(list):
    """The ``events`` list of ``fit`` and a wrapper of its loss log: keeps, on the host, what a snapshot taken after the
    current sequence has to show -- the first generated frame of the sequence (after the first push) and the trainer's last
    window (at the "print" event, which with print_freq 1 follows every sequence, right before the snapshot)."""

    def __init__(self, trainer, log):
        super().__init__()
        self.tr, self.log, self.windows, self.first, self.states = trainer, log, 0, None, []

    def push(self, losses, scaler=None):
        self.log.push(losses, scaler)
        if self.windows == 0:
            self.first = self.tr.last_outputs[0][0, 0].cpu()
        self.windows += 1

    def read(self):
        return self.log.read()

    def append(self, ev):
        super().append(ev)
        if ev[0] == "print":
            from ir2rgb_amd import visuals as V
            t = V.trainer_tensors(self.tr, self.first)
            self.states.append((ev[1], self.windows, {k: (None if v is None else v.cpu().clone()) for k, v in t.items()}))


def _run(dev, snapshots_dir):
    from ir2rgb_amd import fit
    from ir2rgb_amd.losslog import LossLog
    from ir2rgb_amd.schedule import TrainingSchedule
    from ir2rgb_amd.training import loss_names
    from ir2rgb_amd.visuals import Snapshots
    tr = _trainer(dev)
    log = LossLog(dev, loss_names(tr.t_scales))
    watch = _Watch(tr, log)
    s = TrainingSchedule(niter=2, niter_decay=0, niter_step=1, print_freq=1, save_latest_freq=1000, n_frames_total=2,
                         n_scales_spatial=2, seq_len_max=6)
    snaps = Snapshots(dev, snapshots_dir, freq=2, fmt="png") if snapshots_dir is not None else None
    fit(tr, _Sequences(dev, watch), s, log=lambda *_: None, loss_log=watch, events=watch, snapshots=snaps)
    history = {k: log.history(k) for k in log.names}
    checksum = torch.cat([p.detach().double().flatten() for g in tr.netG for p in g.parameters()])
    return tr, watch, snaps, history, checksum


def test_fit_with_snapshots(dev, tmp_path):
    from PIL import Image
    from ir2rgb_amd import visuals as V
    tr, watch, snaps, history, checksum = _run(dev, str(tmp_path))
    # two epochs of two sequences, freq 2: one snapshot per epoch, after its second sequence
    assert snaps.count == 2 and snaps._pending is None and len(watch.states) == 4
    names = [n for n, _, _ in V.panels(watch.states[0][2], tr.opt)]
    assert len(names) == 9 and snaps.names == names
    assert sorted(os.listdir(tmp_path / "images")) == sorted(V.image_name(e, n, "png") for e in (1, 2) for n in names)
    for epoch, state in ((1, watch.states[1]), (2, watch.states[3])):
        assert state[0] == epoch and state[1] >= 2          # (more than one window: the first frame is not the last)
        plist = V.panels(state[2], tr.opt)
        want = V.reference_images(plist)
        for name, kind, x in plist:
            im = Image.open(tmp_path / "images" / V.image_name(epoch, name, "png"))
            assert im.mode == ("L" if x.shape[0] == 1 else "RGB") and im.size == (128, 64)
            got = np.asarray(im)
            if kind == V.FLOW:
                _, decided, _, _ = V.flow_to_rgb_reference(x)
                assert np.array_equal(got[decided], want[name][decided]), (epoch, name)
                assert (got != want[name]).any(-1).mean() < 0.01
            else:
                assert np.array_equal(got, want[name]), (epoch, name, int((got != want[name]).sum()))
        assert not torch.equal(state[2]["fake_B_first"], state[2]["fake_B"][0, -1])
    html = open(tmp_path / "index.html").read()
    assert html.index("epoch [2]") < html.index("epoch [1]") and html.count("<table") == 4
    # the run itself is untouched: every logged value and every generator parameter, bit for bit
    _, _, none, history0, checksum0 = _run(dev, None)
    assert none is None
    for k in history:
        assert torch.equal(history[k].view(torch.int32), history0[k].view(torch.int32)), k
    assert len(history["G"]) == 2 * 2 + 2 * 4 and torch.equal(checksum.view(torch.int64), checksum0.view(torch.int64))
