"""Writes tests/golden/pointwise_bits.json: the sha1 of the bytes of every output the fp64 replays check, per number
format, for the BatchNorm and pointwise kernels of ir2rgb_amd/csrc/pointwise.hip and backward.hip at their edge records
(RECORDS below: every EDGE_BN record and the EDGE records of the x-im2col, its adjoint, the reflection fold, the thin
gradient and the three layout converters), with the sha1 of the operands each replay drew.

    python tests/golden/make_pointwise_bits.py            # on the MI355X, with a library built from a KNOWN-GOOD commit

The table is the yardstick of a refactor of those kernels (tests/test_pointwise_bits_gpu.py: results unchanged to the
bit), so it is never made from the code under test: check out the commit the change starts from, lay the current oracle/
and this file over it, build, run this there and commit the table with the change.  Every record runs twice; a record
whose two runs differ is refused (nothing is written).  The outputs are captured by oracle.replay.digests -- the replays'
own launches, no second set of launch code.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import replay  # noqa: E402
from oracle.edge_records import EDGE, EDGE_BN  # noqa: E402

PATH = os.path.join(HERE, "pointwise_bits.json")
ENTRIES = ("ir2rgb_xexpand", "ir2rgb_xexpand_cx", "ir2rgb_xexpand_bwd", "ir2rgb_fold_reflect", "ir2rgb_thin_grad_expand",
           "ir2rgb_nchw_f32_to_nhwc_half", "ir2rgb_nhwc_half_to_nchw_f32", "ir2rgb_nchw_f32_to_nhwc_half_slice")
RECORDS = EDGE_BN + [r for r in EDGE if r["entry"] in ENTRIES]
IDS = replay.ids(RECORDS)


def capture(dev, rec):
    """-> oracle.replay.digests of the record's replay (which also holds it to its fp64 bound)."""
    if rec["kind"] == "bn":
        from oracle import replay_kernels as RK
        return replay.digests(RK.bn_case, dev, rec, False)
    from oracle import replay_ops as RO
    return replay.digests(RO.REPLAY[rec["entry"]], dev, rec, replay.gen(rec))


def main():
    import torch
    dev = torch.device("cuda:0")
    table = {}
    for name, rec in zip(IDS, RECORDS):
        first, second = capture(dev, rec), capture(dev, rec)
        if first != second:
            raise SystemExit(f"{name}: two runs differ -- nothing written")
        assert first["out"], name
        table[name] = first
    with open(PATH, "w") as f:
        json.dump(table, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(table)} records, {sum(len(v['out']) for v in table.values())} outputs -> {PATH}")


if __name__ == "__main__":
    main()
