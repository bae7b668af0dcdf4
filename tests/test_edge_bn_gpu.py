"""The BatchNorm entry points at small and ragged shapes and in the forms the training window never launches, through
_bn_case of tests/test_window_kernels_gpu.py (fp64 references and bounds of oracle/bn_ref.py, unchanged).

EDGE_BN is a hand-written table in the manifest's record format (``entry``, ``args`` with booleans for pointers), chosen
from the dispatch in ir2rgb_bn_bwd and pointwise.hip:

* ir2rgb_bn_bwd: pixel counts on both sides of the one-launch / two-pass switch (4096 / 4097) and of one 512-pixel slab,
  one and two pixels, C = 2048 on both sides of the 16-channel-group switch (2048 / 2049 pixels); every activation in
  the plain, evaluation-mode (act | 16), accumulating (act | 32) and combined forms; the bias-only form (scale NULL).
* ir2rgb_bn_finalize[_ex]: 1 .. 2049 partial rows (2049: the 8-channel workgroups), channel counts that fill no whole
  group, count 1 (the unbiased-variance guard), stat_updates 1 .. 3, with and without conv_bias, evaluation mode.
* ir2rgb_bn_finalize_apply: the odd row-half split and the 8-row unroll, pixel counts around the 32-row pass and the
  128-pixel chunk, 0 / 1 / 2 residuals, every activation -- and bit-identity with the two-launch path ("two_launch").
* ir2rgb_bn_apply: 8 .. 64 channels, 1 .. 257 pixels.
"""
import importlib.util
import os
import time

import pytest

from oracle import window as WG

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location("_edge_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


K = _load("test_window_kernels_gpu")
TABLE = []
MOM, EPS = 0.1, 1e-05


def bwd(npix, C, act, scale=True):
    s = bool(scale)
    return {"kind": "bn", "entry": "ir2rgb_bn_bwd",
            "args": [True, True, s, s, s, s, True, True, True, True, npix, C, act, 1]}


def finalize(rows, C, count, upd=1, bias=True, frozen=0, entry="ir2rgb_bn_finalize_ex"):
    args = [True, rows, C, count, True, True, bias, True, True, MOM, EPS, True, True, True, True, upd, frozen]
    if entry == "ir2rgb_bn_finalize":
        args = args[:6] + args[7:-1]
    return {"kind": "bn", "entry": entry, "args": args}


def finalize_apply(rows, C, npix, res, act, upd=1):
    return {"kind": "bn", "entry": "ir2rgb_bn_finalize_apply", "two_launch": True,
            "args": [True, rows, C, npix, True, True, True, True, True, MOM, EPS, True, True, True, True, upd, True,
                     res >= 1, res >= 2, True, npix, act, 1]}


def apply(npix, C, res, act):
    return {"kind": "bn", "entry": "ir2rgb_bn_apply", "args": [True, True, True, res >= 1, res >= 2, True, npix, C, act, 1]}


def _records():
    out = []
    # backward: (pixels x form x activation), C alternating 64 / 128
    i = 0
    for npix in (1, 2, 511, 513, 4096, 4097):
        for form in (0, 16, 32, 48):
            for act in (0, 1, 2):
                out.append(bwd(npix, (64, 128)[i % 2], act | form))
                i += 1
    for npix, act in ((1, 1), (2, 2 | 32), (2048, 1), (2049, 2), (2048, 0 | 32), (2049, 1 | 16), (2048, 2 | 48)):
        out.append(bwd(npix, 2048, act))            # 2048 pixels: 16-channel groups; 2049: 8-channel groups
    for npix in (1, 513):
        for C in (64, 512):
            out.append(bwd(npix, C, (1, 2)[C == 512], scale=False))
    out.append(bwd(4097, 64, 2 | 32, scale=False))
    # finalize
    i = 0
    for rows in (1, 2, 127, 129, 1025, 2049):
        for C in (8, 24, 33, 64, 72):
            out.append(finalize(rows, C, 3 * rows + 1, upd=1 + i % 3, bias=i % 2 == 0))
            i += 1
    for C in (8, 33, 64):
        out.append(finalize(1, C, 1, upd=1 + C % 3))            # one value per channel
    out.append(finalize(2049, 264, 4100, upd=2))                # > 256 channels: 32-channel workgroups at any row count
    for C in (8, 257):
        for bias in (True, False):
            out.append(finalize(1, C, 5, bias=bias, frozen=1))
    for rows, C, upd in ((1, 8, 1), (129, 33, 3), (2049, 72, 2)):
        out.append(finalize(rows, C, 2 * rows + 3, upd=upd, entry="ir2rgb_bn_finalize"))
    # finalize + apply
    i = 0
    for rows in (1, 2, 7, 9, 128):
        for npix in (1, 31, 33, 129, 1000):
            out.append(finalize_apply(rows, (192, 64)[i % 2], npix, i % 3, (i // 3) % 3, upd=1 + (i // 9) % 3))
            i += 1
    # apply
    i = 0
    for C in (8, 24, 64):
        for npix in (1, 3, 257):
            out.append(apply(npix, C, i % 3, (i // 3) % 3))
            i += 1
    return out


EDGE_BN = _records()


@pytest.mark.gpu
@pytest.mark.parametrize("rec", EDGE_BN, ids=K._ids(EDGE_BN))
def test_edge_batchnorm_launch(dev, rec):
    t0 = time.perf_counter()
    worst = K._bn_case(dev, rec, shifted=False)
    dt = time.perf_counter() - t0
    TABLE.append((WG.launch_id(rec), worst, dt))
    print(f"\n{WG.launch_id(rec)}: worst err/bound " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()) + f" ({dt:.2f} s)")


def teardown_module(module):
    if TABLE:
        fam = {}
        for name, worst, _ in TABLE:
            f = name.split("-")[0]
            fam[f] = max(fam.get(f, 0.0), max(worst.values()))
        print("\nedge records, worst err/bound per family: " + ", ".join(f"{k} {v:.4f}" for k, v in sorted(fam.items())))
        print(f"edge records: {len(TABLE)} launches, {sum(t for _, _, t in TABLE):.1f} s, slowest "
              f"{max(t for _, _, t in TABLE):.2f} s")
