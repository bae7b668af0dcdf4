"""The BatchNorm entry points at small and ragged shapes and in the forms the training window never launches: bn_case
of oracle/replay_kernels.py (fp64 references and bounds of oracle/bn_ref.py, unchanged) at the EDGE_BN records of
oracle/edge_records.py (which says how they were chosen).
Run with -s for the worst err/bound per family.
"""
import pytest

from oracle import replay
from oracle import replay_kernels as RK
from oracle import window as WG
from oracle.edge_records import EDGE_BN

TABLE = replay.Table()


@pytest.mark.gpu
@pytest.mark.parametrize("rec", EDGE_BN, ids=replay.ids(EDGE_BN))
def test_edge_batchnorm_launch(dev, rec):
    TABLE.run(WG.launch_id(rec), RK.bn_case, dev, rec, False)


def teardown_module(module):
    TABLE.report("edge records")
