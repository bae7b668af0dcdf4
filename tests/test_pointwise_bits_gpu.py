"""Bit stability of the BatchNorm and pointwise kernels (ir2rgb_amd/csrc/pointwise.hip, backward.hip, bn.h): at every
record of tests/golden/make_pointwise_bits.py (every EDGE_BN record; the EDGE records of the x-im2col, its adjoint, the
reflection fold, the thin gradient and the layout converters) each output the fp64 replay checks has, per number format,
the bytes it had when tests/golden/pointwise_bits.json was written -- at the commit before those kernels were rewritten
around shared device functions.  The replays' fp64 bounds say a result is right; this says a refactor moved no bit.
"""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

_spec = importlib.util.spec_from_file_location("make_pointwise_bits", os.path.join(GOLDEN, "make_pointwise_bits.py"))
MK = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(MK)


@pytest.fixture(scope="module")
def table():
    with open(MK.PATH) as f:
        return json.load(f)


def test_table_covers_the_records(table):
    assert sorted(table) == sorted(MK.IDS)
    assert all(v["out"] for v in table.values())


@pytest.mark.gpu
@pytest.mark.parametrize("rec", MK.RECORDS, ids=MK.IDS)
def test_outputs_are_bit_identical_to_the_recorded_ones(dev, table, rec, request):
    want = table[request.node.callspec.id]
    got = MK.capture(dev, rec)
    assert got["in"] == want["in"], "inputs differ: regenerate at a known-good commit"
    assert [n for n, _ in got["out"]] == [n for n, _ in want["out"]], "the replay checks other outputs than recorded"
    moved = [n for (n, a), (_, b) in zip(got["out"], want["out"]) if a != b]
    assert not moved, f"outputs whose bytes changed: {moved}"
