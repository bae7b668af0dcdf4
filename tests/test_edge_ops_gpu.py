"""The non-convolution entry points at small and ragged shapes: the replays of oracle/replay_ops.py at the EDGE records
of oracle/edge_records.py (which says how they were chosen).

Each record goes to the same REPLAY function, fp64 reference and bound (oracle/bounds.py, unchanged) as the window's
launches (tests/test_window_ops_gpu.py); nothing here has a tolerance of its own.  Seeds come from the record.
Run with -s for the worst err/bound per family.
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


def teardown_module(module):
    TABLE.report("edge records")
