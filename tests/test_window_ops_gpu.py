"""Every non-convolution launch of the 512 x 1024 training window, replayed at its recorded geometry against fp64.

One test per ``"kind": "op"`` record of tests/window_geometries.json (oracle/window.py records them), through the replay
functions of oracle/replay_ops.py: the references of oracle/window_ops_ref.py and the bounds of oracle/bounds.py, fixed
before anything runs.  Entries that take a dtype run in bf16 and f16 from one fp64 reference on operands exact in both
formats.  Every element is compared, and what a launch must leave alone is checked too: channels outside a slice, dT
channels >= Cout*KH (zero), loss slots no term names, the pool bytes around each Adam tensor.  Bias gradients and loss
slots must repeat bit for bit.
Run with -s to see the worst err/bound table.
"""
import pytest

from oracle import replay
from oracle import replay_ops as RO
from oracle import window as WG

REPLAYED = [r for r in WG.op_entries() if r["entry"] in RO.REPLAY]
TABLE = replay.Table()


@pytest.mark.gpu
@pytest.mark.parametrize("rec", REPLAYED, ids=replay.ids(REPLAYED))
def test_window_op_launch(dev, rec):
    TABLE.run(WG.launch_id(rec), RO.REPLAY[rec["entry"]], dev, rec, replay.gen(rec))


def teardown_module(module):
    TABLE.report()
