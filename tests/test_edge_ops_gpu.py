"""The non-convolution entry points at small and ragged shapes: the replays of oracle/replay_ops.py at the EDGE records
of oracle/edge_records.py (which says how they were chosen).

Each record goes to the same REPLAY function, fp64 reference and bound (oracle/bounds.py, unchanged) as the window's
launches (tests/test_window_ops_gpu.py); nothing here has a tolerance of its own.  Seeds come from the record.
EDGE ends with EDGE_FLOW, the FlowNet2 operators (cost volume, pixel-space warp, channel norm, with their gradients); the
argument refusals of those entry points are the plain tests below.  Run with -s for the worst err/bound per family.
"""
import pytest
import torch

from oracle import replay
from oracle import replay_ops as RO
from oracle import window as WG
from oracle.edge_records import EDGE, LOSS_GAP

TABLE = replay.Table()


@pytest.mark.gpu
@pytest.mark.parametrize("rec", EDGE, ids=replay.ids(EDGE))
def test_edge_op_launch(dev, rec):
    TABLE.run(WG.launch_id(rec), RO.REPLAY[rec["entry"]], dev, rec, replay.gen(rec))


@pytest.mark.gpu
def test_loss_unnamed_slot_below_the_last_is_zero(dev):
    """include/ir2rgb_hip.h: out[0 .. max slot] are all written -- a slot below the largest named one that no term names
    receives +0 -- and the slots above it are left alone.  LOSS_GAP names slots 0 and 2."""
    from ir2rgb_amd import _lib
    rec = {"kind": "op", "entry": "ir2rgb_loss_multi_fwd", "count": len(LOSS_GAP), "dtype": 1,
           "items": [dict(it, ga=False) for it in LOSS_GAP]}
    ts = RO._loss_tensors(rec, replay.gen(rec), torch.bfloat16, dev)
    res = torch.full((4,), float("nan"), dtype=torch.float32, device=dev)
    part = torch.empty(_lib.lib().ir2rgb_loss_partial_elems(), dtype=torch.float32, device=dev)
    arr = RO._loss_array(rec, ts)
    _lib.check(_lib.lib().ir2rgb_loss_multi_fwd(arr, len(LOSS_GAP), 1, part, res, _lib.current_stream(res)), "loss_multi_fwd")
    torch.cuda.synchronize()
    got = res.cpu()
    assert got[1].item() == 0.0 and not torch.signbit(got[1]), got
    assert torch.isfinite(got[0]) and got[0] > 0 and torch.isfinite(got[2]) and got[2] > 0, got
    assert torch.isnan(got[3]), got


def _rc(entry, *a):
    from ir2rgb_amd import _lib
    ref = next(x for x in a if isinstance(x, torch.Tensor))
    return getattr(_lib.lib(), entry)(*a, _lib.current_stream(ref))


def _untouched(*ts):
    torch.cuda.synchronize()
    return all(bool(torch.isnan(t).all()) for t in ts)


@pytest.mark.gpu
def test_half_cost_volume_refuses_what_it_cannot_run(dev):
    """The argument checks of ir2rgb_correlation_nhwc_half: a refusal returns its code and launches nothing."""
    e = "ir2rgb_correlation_nhwc_half"

    def run(C=128, W=8, lda=None, offa=0, ldb=None, offb=0, shift=0, mode=1):
        lda, ldb = lda or C, ldb or C
        a = torch.zeros(2 * 2 * W * max(lda, ldb) + 8, dtype=torch.bfloat16, device=dev)
        out = replay.sentinel((1, 2, W, 512), torch.bfloat16, dev) if mode else replay.sentinel((1, 441, 2, W), torch.float32, dev)
        rc = _rc(e, a[shift:], lda, offa, a, ldb, offb, out, mode, 512, 32, 0.1, 1, C, 2, W, 1)
        assert _untouched(out), "a refused call wrote its output"
        return rc
    for mode in (0, 1):
        assert run(W=129, mode=mode) == -2
        for C in (64, 192, 384):
            assert run(C=C, mode=mode) == -2, C
        assert run(lda=132, mode=mode) == -1
        assert run(ldb=192, offb=72, mode=mode) == -1
        assert run(shift=1, mode=mode) == -3


@pytest.mark.gpu
def test_correlation_bwd_refuses_stride1_2_and_resample_takes_no_channels(dev):
    f = torch.zeros(1, 2, 6, 7, device=dev)
    gout = torch.zeros(1, 9, 4, 4, device=dev)
    g1, g2 = replay.sentinel(f.shape, torch.float32, dev), replay.sentinel(f.shape, torch.float32, dev)
    assert _rc("ir2rgb_correlation_bwd", f, f, gout, g1, g2, 1, 2, 6, 7, 2, 1, 2, 2, 2) == -2
    assert _untouched(g1, g2)
    flow = torch.zeros(1, 2, 6, 7, device=dev)
    out, gflow = replay.sentinel((1, 1, 6, 7), torch.float32, dev), replay.sentinel(flow.shape, torch.float32, dev)
    assert _rc("ir2rgb_resample2d_fwd", f, flow, out, 1, 0, 6, 7, 1) == 0
    assert _rc("ir2rgb_resample2d_bwd", f, flow, f, out, gflow, 1, 0, 6, 7, 1) == 0
    assert _untouched(out, gflow)


def teardown_module(module):
    TABLE.report("edge records")
