"""Bit stability of kernel families that were rewritten around shared device functions: at every record of the tables
of tests/golden/make_pointwise_bits.py each output the fp64 replay checks has, per number format, the bytes it had when
the table was written -- at the commit before the rewrite.

    pointwise_bits.json  the BatchNorm and pointwise kernels (ir2rgb_amd/csrc/pointwise.hip, backward.hip, bn.h): every
                         EDGE_BN record; the EDGE records of the x-im2col, its adjoint, the reflection fold, the thin
                         gradient and the layout converters
    wgrad_bits.json      the weight-gradient kernels (ir2rgb_amd/csrc/wgrad_mfma.hip): every EDGE_WGRAD record, plain and
                         accumulating (summation order is fixed by the source: a moved bit is a defect)

The replays' fp64 bounds say a result is right; this says a refactor moved no bit.
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
def tables():
    out = {}
    for name in MK.TABLES:
        with open(os.path.join(GOLDEN, name)) as f:
            out[name] = json.load(f)
    return out


def test_table_covers_the_records(tables):
    ids = [rid for _, rid, _ in MK.CASES]
    assert len(set(ids)) == len(ids), "a record id occurs in two tables"
    for name, table in tables.items():
        assert sorted(table) == sorted(rid for t, rid, _ in MK.CASES if t == name), name
        assert all(v["out"] for v in table.values()), name


@pytest.mark.gpu
@pytest.mark.parametrize("table,rid,rec", MK.CASES, ids=[rid for _, rid, _ in MK.CASES])
def test_outputs_are_bit_identical_to_the_recorded_ones(dev, tables, table, rid, rec):
    want = tables[table][rid]
    got = MK.capture(dev, rec)
    assert got["in"] == want["in"], "inputs differ: regenerate at a known-good commit"
    assert [n for n, _ in got["out"]] == [n for n, _ in want["out"]], "the replay checks other outputs than recorded"
    moved = [n for (n, a), (_, b) in zip(got["out"], want["out"]) if a != b]
    assert not moved, f"outputs whose bytes changed: {moved}"
