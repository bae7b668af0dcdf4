"""The edge records (test-only data, nothing here touches a device): hand-written tables in the format of
tests/window_geometries.json at small and ragged shapes, for the replays of oracle/replay_ops.py (EDGE) and
oracle/replay_kernels.bn_case (EDGE_BN).

The window's own geometries (512 x 1024, widths a multiple of 128, H far above 2 * pad) are the least likely to expose
an indexing bug.  A record is ``entry``, then ``args`` with booleans standing for pointers, or the ``items`` / ``tensors``
forms of the losses and Adam.  A record may carry a ``seed`` key, which changes its inputs (oracle.replay.gen): the warp
records do, chosen on the CPU so that the fp64 reference alone has clamped pixels and few pixels in the ambiguity band
(tests/test_edge_refs_cpu.py checks that without a GPU).

EDGE is chosen from the kernels' code: tile tails, pad < H <= 2 * pad (both mirrors of a reflection land near the far
border), one-pixel planes, N > 1, every threshold between two code paths.

EDGE_BN is chosen from the dispatch in ir2rgb_bn_bwd and pointwise.hip:

* ir2rgb_bn_bwd: pixel counts on both sides of the one-launch / two-pass switch (4096 / 4097) and of one 512-pixel slab,
  one and two pixels, C = 2048 on both sides of the 16-channel-group switch (2048 / 2049 pixels); every activation in
  the plain, evaluation-mode (act | 16), accumulating (act | 32) and combined forms; the bias-only form (scale NULL).
* ir2rgb_bn_finalize[_ex]: 1 .. 2049 partial rows (2049: the 8-channel workgroups), channel counts that fill no whole
  group, count 1 (the unbiased-variance guard), stat_updates 1 .. 3, with and without conv_bias, evaluation mode.
* ir2rgb_bn_finalize_apply: the odd row-half split and the 8-row unroll, pixel counts around the 32-row pass and the
  128-pixel chunk, 0 / 1 / 2 residuals, every activation -- and bit-identity with the two-launch path ("two_launch").
* ir2rgb_bn_apply: 8 .. 64 channels, 1 .. 257 pixels.
"""
from oracle.replay_ops import ARGS


def op(entry, seed=None, **kw):
    """A manifest-format record: every pointer of the prototype given (True) unless named False, integers by name."""
    from ir2rgb_amd import _lib
    names = ARGS[entry].split()
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
# slots 0 and 2 named, slot 1 not: see test_loss_unnamed_slot_below_the_last_is_zero (tests/test_edge_ops_gpu.py)
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

# ---------------------------------------------------------------------------------------------------------------------
# BatchNorm
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
