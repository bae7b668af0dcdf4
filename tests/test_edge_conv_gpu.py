"""The convolution forward and weight-gradient kernels in every compiled form, at small and ragged shapes:
replay_forward / replay_wgrad of oracle/replay_kernels.py (fp64 references of oracle/conv_ref.py, per-element bounds
of oracle/bounds.py, both unchanged) at the EDGE_CONV / EDGE_WGRAD records of oracle/edge_records.py, which says which
dispatch threshold each group sits on.  This file has no tolerance of its own.
Run with -s for the per-launch worst err/bound table.
"""
import pytest
import torch

from oracle import conv_ref as R
from oracle import replay
from oracle import replay_kernels as RK
from oracle import window as WG
from oracle.edge_records import EDGE_CONV, EDGE_WGRAD

TABLE = replay.Table()


@pytest.mark.gpu
@pytest.mark.parametrize("rec", EDGE_CONV, ids=replay.ids(EDGE_CONV))
def test_edge_forward_launch(dev, rec):
    TABLE.run(WG.launch_id(rec), RK.replay_forward, dev, rec, kernel=rec["kernel"])


@pytest.mark.gpu
@pytest.mark.parametrize("rec", EDGE_WGRAD, ids=replay.ids(EDGE_WGRAD))
def test_edge_wgrad_launch(dev, rec):
    TABLE.run(WG.launch_id(rec), RK.replay_wgrad, dev, rec, kernel=rec["kernel"])


def pack_jobs():
    """Every distinct (descriptor fields, adjoint) pair of the records: a pad_mode-2 launch packs its zero-padded twin
    with adjoint=True (as replay_forward does)."""
    seen = {}
    for rec in EDGE_CONV + EDGE_WGRAD:
        d = rec["desc"]
        adj = d["pad_mode"] == 2
        twin = dict(d, pad_mode=0) if adj else d
        seen.setdefault((tuple(twin[f] for f in WG.DESC_FIELDS), adj), (twin, R.weight_shape(d), adj))
    return list(seen.values())


@pytest.mark.gpu
@pytest.mark.parametrize("fmt,dtype,dt", replay.DTYPES, ids=[f for f, _, _ in replay.DTYPES])
def test_batched_pack_is_bit_identical(dev, fmt, dtype, dt):
    """ir2rgb_conv2d_pack_batch_run (what the training loop calls after every optimizer step) on all the records'
    weights in one launch -- generic, tiled and adjoint-tiled entries side by side -- against pack_weight, bit for bit."""
    from ir2rgb_amd import conv as C
    g = torch.Generator().manual_seed(11)
    jobs, want = [], []
    for d, shape, adj in pack_jobs():
        desc = RK._desc(d, dt)
        if C._lib.lib().ir2rgb_conv2d_packed_weight_elems(desc) < 0:
            continue        # (weight-gradient-only geometries: channel counts the forward kernels do not take)
        w = torch.randn(shape, generator=g).to(dev)
        want.append(C.pack_weight(desc, w, adjoint=adj))
        jobs.append((desc, w, torch.zeros_like(want[-1]), adj))
    assert len(jobs) > 100
    batch = C.PackBatch(jobs)
    assert batch.nentries > len(jobs)       # (the sub-pixel classes of a transposed weight are entries of their own)
    batch.run()
    torch.cuda.synchronize()
    kinds = set()
    for (desc, w, got, adj), ref in zip(jobs, want):
        assert torch.equal(replay.bits(got), replay.bits(ref)), (fmt, WG.desc_dict(desc), adj)
        kinds.add((bool(desc.transposed), desc.kh * desc.kw > 9, adj))
    assert {(True, False, False), (False, True, False), (False, False, True), (False, False, False)} <= kinds


def teardown_module(module):
    TABLE.report()
