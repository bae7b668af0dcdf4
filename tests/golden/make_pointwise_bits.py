"""Writes the bit tables under tests/golden/ (TABLES below): the sha1 of the bytes of every output the fp64 replays
check, per number format, with the sha1 of the operands each replay drew.

    pointwise_bits.json  the BatchNorm and pointwise kernels of ir2rgb_amd/csrc/pointwise.hip and backward.hip at their edge
                         records: every EDGE_BN record and the EDGE records of the x-im2col, its adjoint, the reflection
                         fold, the thin gradient and the three layout converters
    wgrad_bits.json      the weight-gradient kernels of ir2rgb_amd/csrc/wgrad_mfma.hip at every EDGE_WGRAD record (the plain
                         and the accumulating result)

    python tests/golden/make_pointwise_bits.py TABLE [TABLE ...]     # on the MI355X, with a library built from a KNOWN-GOOD commit

A table is the yardstick of a refactor of its kernels (tests/test_pointwise_bits_gpu.py: results unchanged to the bit), so
it is never made from the code under test: check out the commit the change starts from, lay the current oracle/ and this
file over it, build, run this there and commit the table with the change.  Every record runs twice; a record whose two
runs differ is refused (nothing is written).  The outputs are captured by oracle.replay.digests -- the replays' own
launches, no second set of launch code.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import replay  # noqa: E402
from oracle.edge_records import EDGE, EDGE_BN, EDGE_WGRAD  # noqa: E402

ENTRIES = ("ir2rgb_xexpand", "ir2rgb_xexpand_cx", "ir2rgb_xexpand_bwd", "ir2rgb_fold_reflect", "ir2rgb_thin_grad_expand",
           "ir2rgb_nchw_f32_to_nhwc_half", "ir2rgb_nhwc_half_to_nchw_f32", "ir2rgb_nchw_f32_to_nhwc_half_slice")
TABLES = {"pointwise_bits.json": EDGE_BN + [r for r in EDGE if r["entry"] in ENTRIES],
          "wgrad_bits.json": EDGE_WGRAD}
CASES = [(table, name, rec) for table, recs in TABLES.items() for name, rec in zip(replay.ids(recs), recs)]


def capture(dev, rec):
    """-> oracle.replay.digests of the record's replay (which also holds it to its fp64 bound)."""
    from oracle import replay_kernels as RK
    if rec["kind"] == "bn":
        return replay.digests(RK.bn_case, dev, rec, False)
    if rec["entry"] == "wgrad":
        return replay.digests(RK.replay_wgrad, dev, rec)
    from oracle import replay_ops as RO
    return replay.digests(RO.REPLAY[rec["entry"]], dev, rec, replay.gen(rec))


def main(tables):
    import torch
    if not tables or any(t not in TABLES for t in tables):
        raise SystemExit(f"usage: make_pointwise_bits.py TABLE [TABLE ...], TABLE one of {', '.join(TABLES)}")
    dev = torch.device("cuda:0")
    for name in tables:
        table = {}
        for _, rid, rec in (c for c in CASES if c[0] == name):
            first, second = capture(dev, rec), capture(dev, rec)
            if first != second:
                raise SystemExit(f"{rid}: two runs differ -- nothing written")
            assert first["out"], rid
            table[rid] = first
            print(rid, flush=True)
        path = os.path.join(HERE, name)
        with open(path, "w") as f:
            json.dump(table, f, indent=0, sort_keys=True)
            f.write("\n")
        print(f"{len(table)} records, {sum(len(v['out']) for v in table.values())} outputs -> {path}")


if __name__ == "__main__":
    main(sys.argv[1:])
