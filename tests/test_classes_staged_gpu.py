"""The sub-pixel class launches and the 64-row tile of conv_igemm_body (layers of at most 64 output channels: weight
rows 0..63 only, 32 output channels per wave, a 64-channel epilogue tile) at the smallest shapes at which each can go wrong.

* test_forward_launch: replay_forward of oracle/replay_kernels.py (fp64 reference, the per-element bounds of
  oracle/bounds.py, both element types, statistics rows included) at RECORDS below.  No tolerance of its own.
* test_half_tile_is_bit_identical: y of every record with the 64-row tile against y with IR2RGB_CONV_HALF_TILE=0 (the
  full 128-row tile), torch.equal.  Each side runs in a fresh child process (the switch is read once per process): this
  file run as a script writes the outputs of every record to a file.  Every output accumulates its K-steps in the same
  order in both tiles, so nothing but the BatchNorm partial sums (not compared here, held to fp64 above) may differ.
* test_records_route_as_written (no GPU): the kernel and the statistics rows each record states, against the host queries.

RECORDS, written N x Cin x H x W -> Cout:
  3x3T stride 2 pad 1: 1x64x5x7 -> 72 / 64 / 40 and 2x64x5x7 -> 136, each with output_padding 0, 1 and (0, 1) (classes of
    unequal size), bias and statistics on and off, fp32 output once;
  4x4T stride 2 pad 1: 1x128x5x3 -> 40 / 64 with bias and LeakyReLU (0.2: the discriminators', 0.1: FlowNet2's);
  (4, 1)T stride (2, 1) pad (1, 0): 1x64x5x7 -> 72 / 64 (two classes);
  a one-pixel input; several tiles with a ragged last one and positions next to a row end (9x70 -> 64, 36x37 and
  33x33 -> 1024: 128- and 64-pixel tiles); Cin 192 / 256 (channel chunks wrapping the 2- and 3-stage rings);
  channel-slice outputs as FlowNet2's deconvolutions launch them (entry "fwd": ldy > Cout at co_off, staged and not);
  the single-class kernel at Cout 64 / 40 / 8, 3x3 stride 1 and 4x1 stride 2, at pixel counts that tile_pixels() turns
    into 64-, 128- and 256-pixel tiles (256: >= 256 tiles and >= 40 K-steps), each with a ragged last tile.
"""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import conv_ref as R                                    # noqa: E402
from oracle import replay                                           # noqa: E402
from oracle import replay_kernels as RK                             # noqa: E402
from oracle import window as WG                                     # noqa: E402
from oracle.edge_records import CLASSES, IGEMM, conv                # noqa: E402

SWITCH = "IR2RGB_CONV_HALF_TILE"


def _records():
    t = dict(transposed=1, stride=2)
    out = []
    # 3x3T: (N, Cout) x output_padding; bias / statistics cycle through on-on, off-on, on-off, off-off
    i = 0
    for n, cout in ((1, 72), (1, 64), (1, 40), (2, 136)):
        for op in (0, 1, (0, 1)):
            out.append(conv("classes:64", CLASSES, 64, n, 64, 5, 7, cout, 3, pad=1, output_padding=op, bias=i % 2 == 0,
                            stats=i % 4 < 2, **t))
            i += 1
    out.append(conv("classes:64", CLASSES, 64, 1, 64, 5, 7, 64, 3, pad=1, output_padding=(0, 1), out_f32=1, bias=True, **t))
    # 4x4T with bias and LeakyReLU
    out.append(conv("classes:64", CLASSES, 64, 1, 128, 5, 3, 40, 4, pad=1, bias=True, act=1, **t))
    out.append(conv("classes:64", CLASSES, 64, 1, 128, 5, 3, 64, 4, pad=1, bias=True, act=2, stats=True, **t))
    # (4, 1)T / stride (2, 1): two classes
    for cout in (72, 64):
        out.append(conv("classes:two", CLASSES, 64, 1, 64, 5, 7, cout, (4, 1), transposed=1, stride=(2, 1), pad=(1, 0),
                        bias=True, stats=True))
    # a one-pixel input: four one-pixel classes with output_padding, one output pixel (one class) without
    out.append(conv("classes:1x1-input", CLASSES, 64, 1, 64, 1, 1, 72, 3, pad=1, output_padding=1, bias=True, stats=True, **t))
    out.append(conv("classes:1x1-input", IGEMM, 64, 1, 64, 1, 1, 72, 3, pad=1, bias=True, stats=True, **t))
    # several tiles, a ragged last one, positions next to a row end
    out.append(conv("classes:64", CLASSES, 64, 1, 64, 9, 70, 64, 3, pad=1, bias=True, stats=True, **t))
    out.append(conv("classes:128", CLASSES, 128, 1, 64, 36, 37, 1024, 3, pad=1, stats=True, **t))
    out.append(conv("classes:64-capped", CLASSES, 64, 1, 64, 33, 33, 1024, 3, pad=1, bias=True, stats=True, **t))
    # channel chunks wrapping the rings
    out.append(conv("classes:64", CLASSES, 64, 1, 192, 5, 7, 64, 3, pad=1, output_padding=1, stats=True, **t))
    out.append(conv("classes:64", CLASSES, 64, 1, 256, 5, 7, 72, 3, pad=1, bias=True, stats=True, **t))
    out.append(conv("classes:64", CLASSES, 64, 1, 256, 5, 7, 64, 4, pad=1, bias=True, **t))
    # channel-slice output views (FlowNet2's deconvolutions write into the concatenation buffer)
    out.append(conv("slice:out", CLASSES, 64, 1, 64, 5, 7, 64, 4, pad=1, ldy=200, co_off=8, bias=True, act=2, entry="fwd", **t))
    out.append(conv("slice:out", CLASSES, 64, 2, 64, 5, 7, 40, 4, pad=1, ldy=172, co_off=100, bias=True, entry="fwd", **t))
    out.append(conv("slice:out", CLASSES, 64, 1, 128, 5, 7, 72, 3, pad=1, output_padding=1, ldy=136, co_off=64, stats=True,
                    entry="fwd", **t))
    # the single-class kernel: 3x3 stride 1 pad 1 and 4x1 stride (2, 1) pad (1, 0) at Cout 64 / 40 / 8
    #   64-pixel tiles: 9 x 11 -> 99 and 5 x 11 -> 55 pixels
    for cout in (64, 40, 8):
        out.append(conv("tile:64", IGEMM, 64, 1, 64, 9, 11, cout, 3, pad=1, bias=cout != 40, stats=True))
        out.append(conv("tile:64", IGEMM, 64, 1, 64, 9, 11, cout, (4, 1), stride=(2, 1), pad=(1, 0), bias=cout == 40,
                        stats=cout != 8))
    #   128-pixel tiles from 256 of them on: 150 x 218 = 32 700 pixels, the last tile holds 60
    out.append(conv("tile:128", IGEMM, 128, 1, 64, 150, 218, 40, 3, pad=1, pad_mode=1, bias=True, stats=True))
    out.append(conv("tile:128", IGEMM, 128, 1, 64, 300, 218, 64, (4, 1), stride=(2, 1), pad=(1, 0), stats=True))
    out.append(conv("tile:128", IGEMM, 128, 1, 64, 150, 218, 8, 3, pad=1, bias=True))
    #   256-pixel tiles: >= 256 tiles and >= 40 K-steps.  200 x 328 = 65 600 pixels (the last tile holds 64) at 45 steps;
    #   257 x 256 = 65 792 (a full last tile) at 40
    out.append(conv("tile:256", IGEMM, 256, 1, 320, 200, 328, 8, 3, pad=1, bias=True, stats=True))
    out.append(conv("tile:256", IGEMM, 256, 1, 640, 514, 256, 64, (4, 1), stride=(2, 1), pad=(1, 0), stats=True))
    return out


RECORDS = _records()
IDS = replay.ids(RECORDS)
TABLE = replay.Table()


def _rows(rec):
    """Statistics rows of the record: ceil(pixels / tile) per class (of one launch: per launch)."""
    d, tp = rec["desc"], rec["tile"]
    if rec["kernel"] == IGEMM:
        return -(-d["N"] * d["Hout"] * d["Wout"] // tp)
    rows = 0
    for a in range(d["stride_h"]):
        for b in range(d["stride_w"]):
            hs, ws = -(-(d["Hout"] - a) // d["stride_h"]), -(-(d["Wout"] - b) // d["stride_w"])
            rows += -(-d["N"] * hs * ws // tp)
    return rows


def test_records_route_as_written():
    from ir2rgb_amd import conv as C
    assert os.environ.get(SWITCH) is None
    for rec in RECORDS:
        for _, _, dt in replay.DTYPES:
            desc = RK._desc(rec["desc"], dt)
            assert C.kernel_name(desc) == rec["kernel"], WG.launch_id(rec)
            assert C.stats_rows(desc) == _rows(rec), WG.launch_id(rec)
    couts = {(r["kernel"], r["tile"], min(r["desc"]["Cout"], 65)) for r in RECORDS}
    for tp in (64, 128, 256):       # the 64-row tile at every pixel-tile size of the single-class kernel ...
        assert any(k == IGEMM and t == tp and c <= 64 for k, t, c in couts)
    assert {(CLASSES, 64, 64), (CLASSES, 64, 40), (CLASSES, 64, 65), (CLASSES, 128, 65)} <= couts


@pytest.mark.gpu
@pytest.mark.parametrize("rec", RECORDS, ids=IDS)
def test_forward_launch(dev, rec):
    TABLE.run(WG.launch_id(rec), RK.replay_forward, dev, rec, kernel=rec["kernel"])


def outputs(dev):
    """{record id / format: y (CPU)} of every record, from replay_forward's inputs (statistics requested as recorded)."""
    from ir2rgb_amd import conv as C
    out = {}
    for rid, rec in zip(IDS, RECORDS):
        d = rec["desc"]
        g = replay.gen(rec)
        x = R.draw((d["N"], d["Cin"], d["Hin"], d["Win"]), g)
        w = R.draw(R.weight_shape(d), g, R.weight_scale(d))
        bias = R.draw((d["Cout"],), g).to(dev) if rec["bias"] else None
        for fmt, dtype, dt in replay.DTYPES:
            desc = RK._desc(d, dt)
            wp = C.pack_weight(desc, w.to(dev))
            xd = x.to(dev, dtype).contiguous(memory_format=torch.channels_last)
            if rec["entry"] == "fwd":
                odt = torch.float32 if d["out_f32"] else dtype
                ybuf = torch.zeros((d["N"], d["ldy"], d["Hout"], d["Wout"]), device=dev, dtype=odt)
                ybuf = ybuf.contiguous(memory_format=torch.channels_last)
                stats = torch.zeros((C.stats_rows(desc), 2, d["Cout"]), device=dev) if rec["stats"] else None
                C.conv2d_fwd_view(desc, xd, wp, bias, ybuf, stats)
                y = ybuf
            else:
                y, _ = C.conv2d_fwd(desc, xd, wp, bias, want_stats=rec["stats"])
            torch.cuda.synchronize()
            out[f"{rid} {fmt}"] = y.permute(0, 2, 3, 1).contiguous().cpu()
    return out


@pytest.mark.gpu
def test_half_tile_is_bit_identical(dev, tmp_path):
    files = {}
    for value in ("1", "0"):
        files[value] = str(tmp_path / f"y{value}.pt")
        env = dict(os.environ)
        env[SWITCH] = value
        subprocess.run([sys.executable, os.path.abspath(__file__), files[value]], check=True, env=env, cwd=ROOT, timeout=300)
    new, old = torch.load(files["1"]), torch.load(files["0"])
    assert set(new) == set(old) and len(new) == 2 * len(RECORDS)
    bad = [k for k in new if not torch.equal(replay.bits(new[k]), replay.bits(old[k]))]
    assert not bad, f"y differs between the 64-row and the 128-row tile at {bad}"
    assert all(bool(torch.isfinite(v.float()).all()) and bool(v.float().abs().max() > 0) for v in new.values())


def teardown_module(module):
    TABLE.report()


if __name__ == "__main__":
    torch.save(outputs(torch.device("cuda:0")), sys.argv[1])
