"""Every half-storing kernel family at f16's range edges and on planted inf / NaN: the EDGE_RANGE records of
oracle/edge_records.py in each of their modes (oracle/range_cases.py: overflow, subnormal, nonfinite), through the
``mode`` argument of the replays of oracle/replay_kernels.py and oracle/replay_ops.py and oracle.bounds.check_range.

What is asserted per launch: the reference is live for the mode (tests/test_range_cpu.py checks the same without a
GPU); every output element that must be inf is inf of the right sign, every one that must be finite is inside the
kernel's bound with the rounding term max(u |ref|, 2^-25) and no ETA (so a flushed subnormal fails); where the fp64
reference under torch's semantics is inf / NaN the kernel's result is non-finite too, and nowhere else.  This file has
no tolerance of its own.  Run with -s for the table of worst err/bound and the four counts per launch.
"""
import pytest

from oracle import replay
from oracle import replay_kernels as RK
from oracle import replay_ops as RO
from oracle import window as WG
from oracle.edge_records import RANGE_CASES

pytestmark = pytest.mark.gpu

TABLE = replay.RangeTable()
IDS = [f"{WG.launch_id(r)}-{m}-{(r.get('plant') or ('',))[0]}" for r, m in RANGE_CASES]


@pytest.mark.parametrize("rec,mode", RANGE_CASES, ids=IDS)
def test_range_launch(dev, rec, mode):
    name = WG.launch_id(rec) + (f" plant {rec['plant']}" if mode == "nonfinite" and "plant" in rec else "")
    if rec["kind"] == "conv":
        TABLE.run(name, mode, RK.replay_wgrad if rec["entry"] == "wgrad" else RK.replay_forward, dev, rec)
    elif rec["kind"] == "bn":
        TABLE.run(name, mode, RK.bn_case, dev, rec)
    else:
        TABLE.run(name, mode, RO.REPLAY[rec["entry"]], dev, rec, replay.gen(rec))


def teardown_module(module):
    TABLE.report()
