"""The non-convolution entry points at small and ragged shapes, through the replays of tests/test_window_ops_gpu.py.

The window's own geometries (512 x 1024, widths a multiple of 128, H far above 2 * pad) are the least likely to expose
an indexing bug.  EDGE below is a hand-written table in the manifest's record format -- ``entry``, then ``args`` with
booleans standing for pointers, or the ``items`` / ``tensors`` forms of the losses and Adam -- chosen from the kernels'
code: tile tails, pad < H <= 2 * pad (both mirrors of a reflection land near the far border), one-pixel planes, N > 1,
every threshold between two code paths.  Each record goes to the same REPLAY function, fp64 reference and bound
(oracle/bounds.py, unchanged) as the window's launches; nothing here has a tolerance of its own.  Seeds come from the
record (a record may carry a ``seed`` key: the warp records do, chosen on the CPU so that the fp64 reference alone has
clamped pixels and few pixels in the ambiguity band -- tests/test_edge_refs_cpu.py checks that without a GPU).
Run with -s for the worst err/bound per family.
"""
import importlib.util
import os
import time

import pytest
import torch

from oracle import window as WG

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location("_edge_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _load("test_window_ops_gpu")
TABLE = []


def op(entry, seed=None, **kw):
    """A manifest-format record: every pointer of the prototype given (True) unless named False, integers by name."""
    from ir2rgb_amd import _lib
    names = G.ARGS[entry].split()
    types = _lib.PROTOTYPES[entry][1]
    args = []
    for n, t in zip(names, types):
        if t is _lib.c_void_p:
            args.append(bool(kw.pop(n, True)))
        else:
            args.append(kw.pop(n))
    assert not kw, (entry, kw)
    rec = {"kind": "op", "entry": entry, "args": args}
    if seed is not None:
        rec["seed"] = seed
    return rec


def _heads():
    out = []
    acts = ((273, 1.0), (512, 20.0), (512, 40.0))
    i = 0
    for H in (4, 6, 7, 9, 13):              # 4, 6, 7: pad < H <= 2 * pad;  9, 13: a ragged last 8-row tile
        for W in (1, 5, 17, 33):
            a, mul = acts[i % 3]
            out.append(op("ir2rgb_head_finish", N=2, H=H, W=W, Cout=3, KH=7, CT=24, pad_h=3, acts=a, mul=mul,
                          bias=i % 5 != 4))
            out.append(op("ir2rgb_head_finish_bwd", N=2, H=H, W=W, Cout=3, KH=7, CT=(24, 64)[i % 2], pad_h=3, acts=a,
                          mul=mul, dtype=1))
            i += 1
    # one tap, no padding; and eight channels: no zero-filled dT channels, the LDS limit of the forward (51 KB)
    out.append(op("ir2rgb_head_finish", N=2, H=5, W=19, Cout=1, KH=1, CT=8, pad_h=0, acts=1, mul=1.0))
    out.append(op("ir2rgb_head_finish_bwd", N=2, H=5, W=19, Cout=1, KH=1, CT=8, pad_h=0, acts=1, mul=1.0, dtype=1))
    out.append(op("ir2rgb_head_finish", N=1, H=2, W=3, Cout=1, KH=1, CT=8, pad_h=0, acts=0, mul=20.0))
    out.append(op("ir2rgb_head_finish", N=2, H=9, W=17, Cout=8, KH=7, CT=56, pad_h=3, acts=0x21012012, mul=20.0))
    out.append(op("ir2rgb_head_finish_bwd", N=2, H=9, W=17, Cout=8, KH=7, CT=56, pad_h=3, acts=0x21012012, mul=20.0,
                  dtype=1))
    out.append(op("ir2rgb_head_finish_bwd", N=1, H=4, W=5, Cout=8, KH=7, CT=56, pad_h=3, acts=0x21012012, mul=40.0,
                  dtype=1))
    return out


# (N, Cp, H, W) -> seeds of the backward record and of the forward ones with and without warp_out.  Cp = 3: the warped
# channels are the whole tensor; H or W of 2: every cell is a border cell.  Each seed is the smallest for which the fp64
# reference has a pixel clamped in x, one that is not, and at most 10 % of its pixels in the ambiguity band (a 2 x 2
# image has four pixels and 3 % of them sample beyond the border); tests/test_edge_refs_cpu.py re-checks all three.
WARP_SHAPES = {(1, 3, 2, 2): (16, 0, 2), (2, 6, 3, 5): (0, 2, 0), (1, 9, 7, 2): (0, 0, 2), (3, 6, 17, 33): (0, 0, 0),
               (1, 6, 2, 64): (0, 0, 0)}


def _warps():
    out = []
    for (N, Cp, H, W), seeds in WARP_SHAPES.items():
        out.append(op("ir2rgb_warp_blend_bwd", seed=seeds[0], N=N, Cp=Cp, H=H, W=W))
        for wo, seed in zip((True, False), seeds[1:]):
            out.append(op("ir2rgb_warp_blend_fwd", seed=seed, warp_out=wo, N=N, Cp=Cp, H=H, W=W))
    for N, C, H, W in ((1, 3, 1, 5), (2, 2, 3, 7), (1, 1, 9, 1), (3, 3, 17, 33)):
        for m in range(1, 8):               # every non-empty subset of (warped, diff, norm); 4 = norm only
            out.append(op("ir2rgb_warp_diff_norm_fwd", warped=bool(m & 1), diff=bool(m & 2), norm=bool(m & 4),
                          N=N, C=C, H=H, W=W))
    # (2, 3, 2, 6), (1, 2, 1, 4): H * W a multiple of 4 -- the 16-byte form of the channel norm, with N > 1
    for N, C, H, W in ((1, 3, 1, 5), (2, 2, 3, 7), (1, 1, 9, 1), (3, 3, 17, 33), (2, 3, 2, 6), (1, 2, 1, 4)):
        out.append(op("ir2rgb_channelnorm_fwd", N=N, C=C, H=H, W=W, norm_deg=2))
    return out


def _pools():
    return [op("ir2rgb_avgpool3s2", planes=P, H=H, W=W, backward=b)
            for P, H, W in ((1, 1, 1), (3, 1, 7), (2, 7, 1), (5, 2, 2), (4, 9, 13), (6, 16, 33)) for b in (0, 1)]


def _xexpands():
    """(Cin, KW, stride, pad, mode) x W: column tiles are 128 wide (forward: of Wout, backward: of W)."""
    out = []
    geo = []
    for i, W in enumerate((1, 127, 129, 257)):          # zero padding 3-tap: Wout = W
        geo.append((11 if i % 2 else 6, 3, 1, 1, 0, W))
    for Cin, W in ((9, 4), (6, 4), (9, 129), (6, 127), (6, 257)):   # reflect 7-tap (Cin 9: 63 of 64 channels); W = pad + 1
        geo.append((Cin, 7, 1, 3, 1, W))
    for Cin in (13, 6):                                 # zero padding, stride 2: Wout = W / 2 + 1 = 3, 4, 128, 129
        for W in (5, 6, 254, 256):
            geo.append((Cin, 4, 2, 2, 0, W))
    for i, (Cin, KW, s, p, pm, W) in enumerate(geo):
        N, H = (1, 2)[i % 2], (1, 3)[(i // 2) % 2]
        Wout = (W + 2 * p - KW) // s + 1
        k = dict(N=N, Cin=Cin, H=H, W=W, Wout=Wout, KW=KW, stride_w=s, pad_w=p, pad_mode=pm, dtype=1)
        out.append(op("ir2rgb_xexpand" if i % 3 == 0 else "ir2rgb_xexpand_cx", **(k if i % 3 == 0 else dict(k, Cx=64))))
        out.append(op("ir2rgb_xexpand_bwd", **k))
    for N, H, W in ((2, 3, 5), (1, 1, 257), (1, 3, 256)):   # FlowNetS' first layer: 84 of 128 channels
        out.append(op("ir2rgb_xexpand_cx", N=N, Cin=12, H=H, W=W, Wout=(W + 6 - 7) // 2 + 1, KW=7, stride_w=2, pad_w=3,
                      pad_mode=0, Cx=128, dtype=1))
    return out


def _small():
    out = []
    for N, H, W, C, ph, pw in ((1, 2, 2, 8, 1, 1), (2, 4, 4, 64, 3, 3), (1, 5, 9, 72, 0, 3), (1, 9, 5, 8, 3, 0),
                               (1, 7, 7, 128, 1, 1)):
        out.append(op("ir2rgb_fold_reflect", N=N, H=H, W=W, C=C, pad_h=ph, pad_w=pw, dtype=1))
    for N, Cout, H, W in ((1, 1, 1, 1), (2, 3, 5, 9), (1, 8, 4, 4), (3, 5, 7, 37)):
        out.append(op("ir2rgb_thin_grad_expand", N=N, Cout=Cout, H=H, W=W, dtype=1))
    for N, h, w, ld, off in ((1, 1, 1, 2, 0), (2, 3, 5, 10, 8), (1, 1, 9, 66, 0), (1, 7, 1, 194, 192)):
        for bias in (True, False):
            out.append(op("ir2rgb_flow_upsample_slice", bias=bias, N=N, h=h, w=w, ld=ld, c_off=off, dtype=1))
    for n in (1, 255, 257, 1025):
        out.append(op("ir2rgb_gather_f32", n=n))
    return out


def _item(kind, n, slot, weight=1.0, target=0.0, hw=0, chw=0, b=None, ga=True):
    return {"kind": kind, "n": n, "hw": hw, "chw": chw, "weight": weight, "target": target, "slot": slot,
            "b": (kind != 1) if b is None else b, "ga": ga, "mask": kind == 2}


# 32 items (IR2RGB_LOSS_MAX_ITEMS) of all three kinds in one launch: every small item gets exactly one block, n = 2056
# two, the 300 000-element item one per 2048 elements.  Kind 2 with C = 1 (chw == hw), N = 3, and b NULL.
LOSS_ITEMS = [
    _item(1, 1, 0, 1.0, 1.0), _item(0, 8, 1, 5.0), _item(1, 2056, 0, 2.0, 1.0), _item(2, 35, 2, 10.0, hw=35, chw=35),
    _item(2, 135, 3, 10.0, hw=15, chw=45), _item(2, 72, 2, 5.0, hw=12, chw=36, b=False), _item(0, 300000, 1, 5.0),
    _item(1, 2, 0), _item(1, 3, 1, 1.0, 1.0), _item(1, 255, 0, 2.0), _item(1, 257, 1, 1.0, 1.0), _item(1, 2047, 3),
    _item(1, 2048, 0, 1.0, 1.0), _item(1, 2049, 2), _item(1, 4097, 1, 2.0, 1.0), _item(0, 16, 1, 5.0),
    _item(0, 2040, 3, 5.0), _item(0, 2048, 1, 10.0), _item(0, 2056, 2, 5.0), _item(0, 4104, 1, 5.0),
    _item(0, 8, 0, 1.0, ga=False), _item(0, 24, 3, 5.0), _item(2, 1, 0, 5.0, hw=1, chw=1),
    _item(2, 6, 1, 5.0, hw=1, chw=3), _item(2, 2058, 2, 10.0, hw=343, chw=1029), _item(2, 2049, 3, 10.0, hw=683, chw=2049),
    _item(2, 510, 0, 10.0, hw=85, chw=255, b=False), _item(1, 5, 2, 1.0, 1.0), _item(1, 8191, 3), _item(0, 8200, 0, 5.0),
    _item(2, 4096, 1, 10.0, hw=2048, chw=4096), _item(1, 1023, 2, 2.0, 1.0, ga=False),
]
# slots 0 and 2 named, slot 1 not: see test_loss_unnamed_slot_below_the_last_is_zero
LOSS_GAP = [_item(1, 77, 0, 1.0, 1.0), _item(0, 264, 2, 5.0), _item(2, 90, 2, 10.0, hw=15, chw=45)]


def _losses():
    out = []
    for items in (LOSS_ITEMS, LOSS_GAP):
        fwd = [dict(it, ga=False) for it in items]
        out.append({"kind": "op", "entry": "ir2rgb_loss_multi_fwd", "count": len(items), "dtype": 1, "items": fwd})
        out.append({"kind": "op", "entry": "ir2rgb_loss_multi_bwd", "count": len(items), "dtype": 1, "items": items})
    return out


# the chunk boundary ir2rgb_adam_chunk_elems() = 8192, the n % 4 tail of the last chunk, a single partial chunk; each n
# with every array 16-byte aligned and at a 4-byte offset
ADAM_NS = (1, 2, 3, 5, 8191, 8192, 8193, 16387)
ADAM = {"kind": "op", "entry": "ir2rgb_adam_step", "lr": 0.0002, "beta1": 0.5, "beta2": 0.999, "eps": 1e-08,
        "nblocks": 2 * sum(-(-n // 8192) for n in ADAM_NS), "tensors": [[n, al, 1] for n in ADAM_NS for al in (False, True)]}

EDGE = _heads() + _warps() + _pools() + _xexpands() + _small() + _losses() + [ADAM]


def gen(rec):
    """The record's generator: _gen of the window replays (a crc of the whole record, its seed key included)."""
    return G._gen(rec)


@pytest.mark.gpu
@pytest.mark.parametrize("rec", EDGE, ids=G._ids(EDGE))
def test_edge_op_launch(dev, rec):
    t0 = time.perf_counter()
    worst = G.REPLAY[rec["entry"]](dev, rec, gen(rec))
    dt = time.perf_counter() - t0
    TABLE.append((WG.launch_id(rec), worst, dt))
    print(f"\n{WG.launch_id(rec)}: worst err/bound " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()) + f" ({dt:.2f} s)")


@pytest.mark.gpu
def test_loss_unnamed_slot_below_the_last_is_zero(dev):
    """include/ir2rgb_hip.h: out[0 .. max slot] are all written -- a slot below the largest named one that no term names
    receives +0 -- and the slots above it are left alone.  LOSS_GAP names slots 0 and 2."""
    from ir2rgb_amd import _lib
    rec = {"kind": "op", "entry": "ir2rgb_loss_multi_fwd", "count": len(LOSS_GAP), "dtype": 1,
           "items": [dict(it, ga=False) for it in LOSS_GAP]}
    ts = G._loss_tensors(rec, gen(rec), torch.bfloat16, dev)
    res = torch.full((4,), float("nan"), dtype=torch.float32, device=dev)
    part = torch.empty(_lib.lib().ir2rgb_loss_partial_elems(), dtype=torch.float32, device=dev)
    arr = G._loss_array(rec, ts)
    _lib.check(_lib.lib().ir2rgb_loss_multi_fwd(arr, len(LOSS_GAP), 1, part, res, _lib.current_stream(res)), "loss_multi_fwd")
    torch.cuda.synchronize()
    got = res.cpu()
    assert got[1].item() == 0.0 and not torch.signbit(got[1]), got
    assert torch.isfinite(got[0]) and got[0] > 0 and torch.isfinite(got[2]) and got[2] > 0, got
    assert torch.isnan(got[3]), got


def teardown_module(module):
    if TABLE:
        fam = {}
        for name, worst, _ in TABLE:
            f = name.split("-")[0]
            fam[f] = max(fam.get(f, 0.0), max(worst.values()))
        print("\nedge records, worst err/bound per family: " + ", ".join(f"{k} {v:.4f}" for k, v in sorted(fam.items())))
        print(f"edge records: {len(TABLE)} launches, {sum(t for _, _, t in TABLE):.1f} s, slowest "
              f"{max(t for _, _, t in TABLE):.2f} s")
