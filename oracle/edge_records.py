"""The edge records (test-only data, nothing here touches a device): hand-written tables in the format of
tests/window_geometries.json at small and ragged shapes, for the replays of oracle/replay_ops.py (EDGE, which ends
with EDGE_FLOW) and of oracle/replay_kernels.py: bn_case (EDGE_BN), replay_forward (EDGE_CONV) and replay_wgrad (EDGE_WGRAD).
EDGE_RANGE, at the end of the file with its own table of which record reaches which half store, reuses the smallest of
them for the ``mode=`` of those replays: f16's overflow and subnormal edges and planted inf / NaN (oracle/range_cases.py).

The window's own geometries (512 x 1024, widths a multiple of 128, H far above 2 * pad) are the least likely to expose
an indexing bug.  A record is ``entry``, then ``args`` with booleans standing for pointers, or the ``items`` / ``tensors``
forms of the losses and Adam.  A record may carry a ``seed`` key, which changes its inputs (oracle.replay.gen): the warp
records do, chosen on the CPU so that the fp64 reference alone has clamped pixels and few pixels in the ambiguity band
(tests/test_edge_refs_cpu.py checks that without a GPU).

EDGE is chosen from the kernels' code: tile tails, pad < H <= 2 * pad (both mirrors of a reflection land near the far
border), one-pixel planes, N > 1, every threshold between two code paths.

The layout converters (pointwise.hip: 64-pixel x 64-channel LDS tiles) run at 1, 63, 64, 65 and 129 pixels times 1, 3,
63, 64 and 65 channels with N = 2, the slice form with ld > C, an odd c_off and both activations.

EDGE_FLOW (the FlowNet2 operators) is chosen from correlation.hip, correlation_mfma.hip, resample2d.hip and
channelnorm.hip.  A record names its ``form`` (FLOW_FORMS) by hand; for the forward cost volume corr_form restates the
dispatch of ir2rgb_correlation_fwd and tests/test_edge_flow_cpu.py holds the two against each other.  Keys beside the
arguments: ``offset`` {tensor: elements} (a misaligned base pointer), ``far`` [fx, fy] (added to every flow vector),
``scale`` (of the channel norm's input), ``modes`` (the out modes of the half-precision cost volume).

* corr_fwd_lds (fast parameters (20, 1, 20, 1, 2), C % 8 == 0), one thing varied from (1, 16, 5, 24): C = 8 / 16 / 24
  (two / one / none of the three prologue stages is the no-op form), 32 (the ring exactly full) and 40 (its first
  wrap); W = 8 (one live lane in 16), 128, 136 (a second x chunk of one lane); H = 1 (20 of 21 workgroups skip the
  pipeline), 2, 3 and 41 (the middle row has all 21 tj rows valid); N = 2, 3; a grid that is a multiple of 8 (the XCD
  renumbering) beside ones that are not.
* corr_fwd_tile (C % 8 != 0): C = 1, 3, 5, 7 (lane quarters and channel halves that own no channel), 9, 17; W = 8 and
  136, H = 1 and 41, N = 2.
* corr_fwd_generic: the fast parameters at W % 8 != 0 and with in1 or out one element off alignment; k = 3 at stride1 =
  2 with an odd extent (the ceil), pad = 0, pad < md, pad > md, md % stride2 != 0, stride2 = 1, N = 2, a one-pixel output.
* corr_bwd_kernel: the fast parameters, k = 3, pad on both sides of md, stride2 = 1 and 3.
* corr_mfma_kernel (both dtypes and both out modes per record): C = 128 / 256, W = 1 (parity 1 owns no pixel), 2 and
  the widths around the 16-pixel blocks of a parity (31 .. 33, 63, 65, 127, 128), H = 1 (the lower-half workgroups only
  zero-flush), 2, 3, 21 and 41 (all 21 rows valid, five wraps of the 4-row ring), N * H odd and even (the XCD
  renumbering), channel-slice views of a, b and out, slope 1 / 0.1 / 0.
* resample2d: one-row, one-column, one-pixel planes, N > 1, and ``far`` records whose pixels all land on one border
  column / row (the atomics' long chain, both corners of an axis on one pixel, the truncation weights below zero).
* channelnorm_bwd: the forward's shapes (each with an all-zero pixel) and an input of 1e-8, where the 1e-9 of the
  denominator is a tenth of the norm.

EDGE_BN is chosen from the dispatch in ir2rgb_bn_bwd and pointwise.hip:

* ir2rgb_bn_bwd: pixel counts on both sides of the one-launch / two-pass switch (4096 / 4097) and of one 512-pixel slab,
  one and two pixels, C = 2048 on both sides of the 16-channel-group switch (2048 / 2049 pixels); every activation in
  the plain, evaluation-mode (act | 16), accumulating (act | 32) and combined forms; the bias-only form (scale NULL).
* ir2rgb_bn_finalize[_ex]: 1 .. 2049 partial rows (2049: the 8-channel workgroups), channel counts that fill no whole
  group, count 1 (the unbiased-variance guard), stat_updates 1 .. 3, with and without conv_bias, evaluation mode.
* ir2rgb_bn_finalize_apply: the odd row-half split and the 8-row unroll, pixel counts around the 32-row pass and the
  128-pixel chunk, 0 / 1 / 2 residuals, every activation -- and bit-identity with the two-launch path ("two_launch").
* ir2rgb_bn_apply: 8 .. 64 channels, 1 .. 257 pixels.

EDGE_CONV ("kind": "conv", entries "fwd_ws" / "fwd") is chosen from the forward dispatch.  Each record names its
``form`` (CONV_FORMS) and states by hand the ``kernel`` that runs, whether a ``workspace`` is wanted and the ``tile`` of a
statistics row; tests/test_edge_conv_cpu.py holds the library's host queries against all three.

* tile_pixels (conv_mfma.hip): 64-, 128- and 256-pixel tiles, each with a ragged last pixel tile and a ragged channel
  tile (Cout 72 / 136 / 200 / 1000); both sides of 256 tiles of 128 pixels (P = 3968 / 3969 at Cout = 1024) and of 256
  tiles of 256 pixels with >= 40 K-steps (P = 7936 / 8001, 4x4 at Cin = 192).
* launch_conv: every fixed tap template at stride 2 on 9 x 11, the runtime-tap form (5x5, 3x1, 7x7 = IR2RGB_MAX_TAPS),
  the THIN forms (Cout <= 32 with 4x4 and 1x7) and Cout = 33 beside them.
* the epilogue of conv_igemm_body: scalar stores (Cout % 4 != 0), 8-byte stores (Cout % 8 != 0), the staged form, fp32
  output, every activation, bias and statistics present and absent, stats_per_sample with tiles cut inside a sample.
* make_plan's channel slices ("fwd": conv2d_fwd_view): ldx > Cin at ci_off 8 / 64, ldy > Cout at co_off 8 / 100 / 192,
  an odd co_off with Cout % 4 != 0.  The replay asserts that nothing outside the slice is written.
* borders: reflection with pad < H <= 2 * pad per axis, Hout / Wout / the whole output of one pixel, zero padding
  larger than the image, a tile that spans two samples.
* make_plan's sub-pixel classes and launch_classes: 3x3 (output_padding 0 / 1 / mixed) and 4x4 at stride 2,
  4x1 at stride (2, 1) (two classes), odd outputs (classes of different Hsub / Wsub), a 1 x 1 input, per-class
  workgroup counts of 1 and 2 (the (nwg + 7) & ~7 padding blocks), thin Cout, tp_all = 64, 64 because wg128 <= 320,
  and 128; a transposed layer with a single class (stride 1, and the 1 x 1 output) runs conv_igemm_kernel.
* conv_dot_ok (through conv_route): Cin 512 / 1024, 1x1 / 4x4, P = 1, 3, 5, 18 and 8195 (over the 8192-wave cap), a
  channel-slice input; with statistics conv_route sends the same descriptor to conv_igemm_kernel (``named`` keeps what
  the query, which asks conv_route for a launch without bias and statistics, answers).
* conv3x3p_plan (conv3x3_patch.hip): variants 1 .. 4, each at padding 0, 1 and 2 (2 also reflected: two pixels deep),
  pad_mode 0 / 1 / 2, odd Hout, 200 tiles against 199 (conv_igemm_kernel); variants 3 and 4 through the workspace of
  "fwd_ws".
* conv1x7_thin_plan: Cin 64 / 128, Cout 1 .. 32 (1 and 3 inside ldy = 4: the plan wants ldy % 4 == 0), W = 4, 5, 127,
  129, 514 segments on 512 workgroups; with a bias or statistics conv_route takes the general kernel.
* conv7x1_col_plan: Cout 64 / 128, H = 4, 7, 9, W = 1, 31, 33, N = 2, a channel slice, 540 tiles on 512 workgroups.

EDGE_WGRAD (entry "wgrad"; ``splits`` = workspace slabs of the plain call, 0 = written directly) from wgrad_mfma.hip.
replay_wgrad runs every record plain and accumulating; the accumulating call of a nine-tap record takes the one-tap
kernel (wgrad_route), so each of those records covers both.

* plan: tpb = 2 with an odd tap count (3x3 at Cb <= 64) against tpb = 1, Ca / Cb of 8 .. 200, Q = 35 < 64 and
  Q % 64 != 0, a geometry the cost model splits (16 and 8 slabs) and ones it cannot (< 8 K-steps), stride 2 on odd
  sizes, transposed stride 2 with output_padding 0 / 1, reflection with pad < H <= 2 * pad, N = 3.
* launch_wgrad_finish: <= 16 taps (tiled), 25 / 49 taps (the gather form), > 64 splits (wide).
* plan9: Win = 64 / 128 / 192, H = 2 and odd H, ksplit == 1 (Q / 64 < 16: direct write) and > 1 (wgrad_sum_kernel),
  pad_mode 0 / 1, N = 2, 128 -> 192 channels.
* plan_line (which picks launch_line's LineForm): 7x1 at stride 1 (column kernel) and 2 (line kernel), 4x1 at stride 2 (column) and 1 (line),
  1x7, 3x3 / stride 2 with tl = 1, 2, 128 (also transposed) and tl = 4 (the one-tap kernel); Wq % 64 != 0, fewer than
  8 K-steps, a short last split, 65 splits, reflection on the taps' axis with pad < H <= 2 * pad.
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


# H x W of 1, 63, 64, 65 and 129 pixels (the converters' tiles are 64 pixels x 64 channels)
CONVERT_HW = ((1, 1), (7, 9), (8, 8), (5, 13), (3, 43))
CONVERT_C = (1, 3, 63, 64, 65)


def _converters():
    out = []
    for H, W in CONVERT_HW:
        for C in CONVERT_C:
            out.append(op("ir2rgb_nchw_f32_to_nhwc_half", N=2, C=C, H=H, W=W, dtype=1))
            out.append(op("ir2rgb_nhwc_half_to_nchw_f32", N=2, C=C, H=H, W=W, dtype=1))
    # the slice form: ld > C, an odd c_off, both activations (the replay checks the neighbouring channels untouched)
    for i, ((H, W), C) in enumerate(zip(CONVERT_HW + CONVERT_HW, CONVERT_C + CONVERT_C[::-1])):
        out.append(op("ir2rgb_nchw_f32_to_nhwc_half_slice", N=2, C=C, H=H, W=W, ld=C + 8 + i, c_off=(1, 3, 7)[i % 3],
                      act=(0, 2)[i % 2], dtype=1))
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

# ---------------------------------------------------------------------------------------------------------------------
# FlowNet2 operators
FAST = dict(pad_size=20, kernel_size=1, max_displacement=20, stride1=1, stride2=2)
FLOW_FORMS = (
    "lds:ng1", "lds:ng2", "lds:ng3", "lds:ng4", "lds:wrap", "lds:ng2+xcd", "tile:c<8", "tile", "generic:w%8",
    "generic:unaligned", "generic:params",
    "bwd:fast", "bwd:k3", "bwd:pad<md", "bwd:pad>md", "bwd:s2",
    "mfma:kc4", "mfma:kc8", "mfma:w", "mfma:h", "mfma:n", "mfma:slice", "mfma:slope",
    "resample", "resample:far", "channelnorm_bwd", "channelnorm_bwd:tiny",
)


def corr_form(N, C, H, W, pad, k, md, s1, s2, aligned=True):
    """The kernel ir2rgb_correlation_fwd launches (its dispatch in correlation.hip) and, for corr_fwd_lds, how many 8-channel
    stages its 4-stage ring sees and whether the grid is renumbered over the XCDs (a multiple of 8 workgroups)."""
    fast = k == 1 and s1 == 1 and pad == md and s2 == 2 and md // s2 == 10 and md == 20 and W % 8 == 0 and aligned and C > 0
    if not fast:
        if (k, s1, pad, md, s2) == (1, 1, 20, 20, 2) and C > 0:
            return "generic:w%8" if W % 8 else "generic:unaligned"
        return "generic:params"
    if C % 8 == 0 and N * C * H * W * 4 < 2 ** 31:
        ng = C // 8
        xcd = "+xcd" if (N * H * 21 * -(-W // 128)) % 8 == 0 else ""
        return (f"lds:ng{ng}" if ng <= 4 else "lds:wrap") + xcd
    return "tile:c<8" if C < 8 else "tile"


def flow(entry, form, seed=None, offset=None, far=None, scale=None, modes=None, **kw):
    assert form in FLOW_FORMS, form
    rec = op(entry, seed, **kw)
    rec["form"] = form
    for key, v in (("offset", offset), ("far", far), ("scale", scale), ("modes", modes)):
        if v is not None:
            rec[key] = v
    return rec


def _corr_fwd():
    e = "ir2rgb_correlation_fwd"
    out = []
    lds = [(1, 8, 5, 24, "lds:ng1"), (1, 16, 5, 24, "lds:ng2"), (1, 24, 5, 24, "lds:ng3"), (1, 32, 5, 24, "lds:ng4"),
           (1, 40, 5, 24, "lds:wrap"),
           (1, 16, 5, 8, "lds:ng2"), (1, 16, 5, 128, "lds:ng2"), (1, 16, 5, 136, "lds:ng2"),
           (1, 16, 1, 24, "lds:ng2"), (1, 16, 2, 24, "lds:ng2"), (1, 16, 3, 24, "lds:ng2"), (1, 16, 41, 24, "lds:ng2"),
           (2, 16, 5, 24, "lds:ng2"), (3, 16, 5, 24, "lds:ng2"),
           (2, 16, 2, 136, "lds:ng2+xcd")]                  # 2 * 2 * 21 * 2 = 168 workgroups
    tile = [(1, C, 5, 24, "tile:c<8" if C < 8 else "tile") for C in (1, 3, 5, 7, 9, 17)] + \
           [(1, 9, 5, 8, "tile"), (1, 9, 5, 136, "tile"), (1, 9, 1, 24, "tile"), (1, 9, 41, 24, "tile"), (2, 9, 5, 24, "tile")]
    for N, C, H, W, form in lds + tile + [(1, 4, 5, 7, "generic:w%8"), (1, 4, 5, 12, "generic:w%8")]:
        out.append(flow(e, form, N=N, C=C, H=H, W=W, **FAST))
    for name in ("in1", "out"):
        out.append(flow(e, "generic:unaligned", offset={name: 1}, N=1, C=8, H=5, W=24, **FAST))
    for N, C, H, W, pad, k, md, s1, s2 in (
            (1, 3, 7, 9, 3, 3, 3, 2, 3),        # k = 3, stride1 = 2: ceil(5 / 2) x ceil(7 / 2) outputs
            (1, 3, 9, 8, 0, 1, 2, 1, 1),        # pad = 0
            (1, 3, 8, 9, 1, 1, 3, 1, 1),        # pad < md
            (1, 3, 5, 6, 4, 1, 2, 1, 2),        # pad > md
            (1, 3, 5, 6, 3, 1, 3, 1, 2),        # md % stride2 != 0
            (1, 3, 5, 6, 2, 1, 2, 1, 1),        # stride2 = 1
            (2, 3, 5, 6, 2, 1, 2, 1, 2),        # N = 2
            (1, 2, 1, 1, 1, 1, 1, 1, 1)):       # one output pixel
        out.append(flow(e, "generic:params", N=N, C=C, H=H, W=W, pad_size=pad, kernel_size=k, max_displacement=md,
                        stride1=s1, stride2=s2))
    return out


def _corr_bwd():
    e = "ir2rgb_correlation_bwd"
    out = [flow(e, "bwd:fast", N=N, C=C, H=H, W=W, **FAST) for N, C, H, W in ((1, 2, 3, 5), (2, 3, 5, 8))]
    for form, pad, k, md, s2 in (("bwd:k3", 2, 3, 2, 2), ("bwd:pad<md", 1, 1, 2, 2), ("bwd:pad>md", 3, 1, 2, 2),
                                 ("bwd:s2", 3, 1, 3, 1), ("bwd:s2", 3, 1, 3, 3)):
        out.append(flow(e, form, N=1, C=2, H=6, W=7, pad_size=pad, kernel_size=k, max_displacement=md, stride1=1, stride2=s2))
    return out


def _corr_mfma():
    def rec(form, N=1, C=128, H=3, W=8, a=None, b=None, o=(512, 32), slope=0.1):
        (lda, offa), (ldb, offb) = a or (C, 0), b or (C, 0)
        return flow("ir2rgb_correlation_nhwc_half", form, modes=[0, 1], lda=lda, offa=offa, ldb=ldb, offb=offb, out_mode=1,
                    ldo=o[0], offo=o[1], slope=slope, N=N, C=C, H=H, W=W, dtype=1)
    out = [rec("mfma:kc4"), rec("mfma:kc8", C=256)]
    out += [rec("mfma:w", H=2, W=W, C=(128, 256)[i % 2]) for i, W in enumerate((1, 2, 31, 32, 33, 63, 65, 127, 128))]
    out += [rec("mfma:h", H=H) for H in (1, 2, 21, 41)]
    out += [rec("mfma:n", N=2), rec("mfma:n", N=3), rec("mfma:n", N=2, H=1), rec("mfma:n", N=3, H=2, W=33)]
    out += [rec("mfma:slice", a=(192, 64)), rec("mfma:slice", b=(200, 8)), rec("mfma:slice", C=256, b=(320, 64), W=33),
            rec("mfma:slice", C=256, a=(320, 64), b=(328, 8), o=(448, 7), N=2, W=31),
            rec("mfma:slice", o=(441, 0), W=33), rec("mfma:slice", o=(448, 7))]
    out += [rec("mfma:slope", slope=1.0, W=33), rec("mfma:slope", slope=0.0, W=33)]
    return out


RESAMPLE_SHAPES = ((1, 3, 1, 5), (2, 2, 3, 7), (1, 1, 9, 1), (1, 1, 1, 1), (3, 3, 17, 33))
FAR = ([100.0, 0.0], [0.0, -100.0])             # every pixel beyond the right border / above the top one


def _resamples():
    out = []
    for e in ("ir2rgb_resample2d_fwd", "ir2rgb_resample2d_bwd"):
        out += [flow(e, "resample", N=N, C=C, H=H, W=W, kernel_size=1) for N, C, H, W in RESAMPLE_SHAPES]
        out += [flow(e, "resample:far", far=far, N=1, C=2, H=8, W=64, kernel_size=1) for far in FAR]
    return out


def _channelnorm_bwds():
    e = "ir2rgb_channelnorm_bwd"
    out = [flow(e, "channelnorm_bwd", N=N, C=C, H=H, W=W, norm_deg=2)
           for N, C, H, W in ((1, 3, 1, 5), (2, 2, 3, 7), (1, 1, 9, 1), (3, 3, 17, 33), (2, 3, 2, 6), (1, 2, 1, 4))]
    out.append(flow(e, "channelnorm_bwd:tiny", scale=1e-8, N=2, C=3, H=3, W=7, norm_deg=2))
    return out


EDGE_FLOW = _corr_fwd() + _corr_bwd() + _corr_mfma() + _resamples() + _channelnorm_bwds()

EDGE = _heads() + _warps() + _pools() + _xexpands() + _small() + _converters() + _losses() + [ADAM] + EDGE_FLOW

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

# ---------------------------------------------------------------------------------------------------------------------
# Convolution forward and weight gradient.  ``kernel``, ``workspace``, ``tile`` / ``splits`` and ``form`` are the
# expectation, written by hand from the dispatch code; tests/test_edge_conv_cpu.py holds the library's host queries
# against them.
IGEMM, CLASSES, DOT = "conv_igemm_kernel", "conv_igemm_classes_kernel", "conv_dot_kernel"
PATCH, THIN7, COL7 = "conv3x3_patch_kernel", "conv1x7_thin_kernel", "conv7x1_col_kernel"

CONV_FORMS = (
    "tile:64", "tile:128", "tile:256", "tile:127-tiles", "tile:255-tiles",
    "taps:3x3", "taps:4x4", "taps:7x1", "taps:1x7", "taps:4x1", "taps:2x2", "taps:2x1", "taps:1x2", "taps:1x1",
    "taps:runtime", "thin:4x4", "thin:1x7", "thin:33",
    "store:scalar", "store:vector", "store:f32", "act", "stats:per-sample",
    "slice:in", "slice:out", "slice:odd",
    "border:reflect-deep", "border:one-pixel", "border:overpad", "border:two-samples",
    "classes:64", "classes:64-capped", "classes:128", "classes:two", "classes:1x1-input", "classes:thin",
    "transposed:one-class",
    "dot", "dot:capped", "dot:slice", "dot:stats",
    "patch:1", "patch:2", "patch:3", "patch:4", "patch:adjoint", "patch:200-tiles", "patch:199-tiles",
    "thin1x7", "thin1x7:slice", "thin1x7:wrap", "thin1x7:bias",
    "col7x1", "col7x1:wrap",
)
WGRAD_FORMS = (
    "onetap:tpb2", "onetap:tpb1", "onetap:split", "onetap:stride2", "onetap:transposed", "onetap:reflect-deep",
    "onetap:gather-finish", "onetap:tl4",
    "nine:direct", "nine:split",
    "line:col7", "line:line7", "line:col4", "line:line4", "line:1x7", "line:3x3s2", "line:3x3s2-transposed",
    "line:one-split", "line:short-last-split", "line:wide-finish", "line:reflect-deep",
)


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def geometry(N, Cin, H, W, Cout, k, stride=1, pad=0, pad_mode=0, transposed=0, output_padding=0, act=0, out_f32=0, ldx=0,
             ci_off=0, ldy=0, co_off=0, sps=0):
    """A descriptor in the manifest's format (every field of oracle.window.DESC_FIELDS), Hout / Wout filled in."""
    (kh, kw), (sh, sw), (ph, pw) = _pair(k), _pair(stride), _pair(pad)
    oh, ow = _pair(output_padding)
    if transposed:
        Ho, Wo = (H - 1) * sh - 2 * ph + kh + oh, (W - 1) * sw - 2 * pw + kw + ow
    else:
        Ho, Wo = (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1
    return {"N": N, "Hin": H, "Win": W, "Cin": Cin, "Hout": Ho, "Wout": Wo, "Cout": Cout, "kh": kh, "kw": kw, "stride_h": sh,
            "stride_w": sw, "pad_h": ph, "pad_w": pw, "pad_mode": pad_mode, "transposed": transposed, "dtype": 1, "act": act,
            "out_f32": out_f32, "ldx": ldx, "ci_off": ci_off, "ldy": ldy, "co_off": co_off, "stats_per_sample": sps}


def conv(form, kernel, tile, *geo, entry="fwd_ws", bias=False, stats=False, workspace=False, named=None, seed=None, **kw):
    """A forward record.  ``tile``: the pixels of a statistics row -- an integer for the implicit-GEMM kernels
    (tile_pixels), (rows, columns) for the patch and column kernels.  ``named``: what ir2rgb_conv2d_kernel_name answers
    where the launch's bias / statistics arguments, which the query does not see, send it to another kernel."""
    assert form in CONV_FORMS, form
    rec = {"kind": "conv", "entry": entry, "desc": geometry(*geo, **kw), "kernel": kernel, "bias": bias, "stats": stats,
           "workspace": workspace, "form": form, "tile": tile}
    if named is not None:
        rec["named"] = named
    if seed is not None:
        rec["seed"] = seed
    return rec


def wgrad(form, kernel, splits, *geo, **kw):
    """A weight-gradient record.  ``splits``: the slabs of the plain call's workspace (0: written directly)."""
    assert form in WGRAD_FORMS, form
    return {"kind": "conv", "entry": "wgrad", "desc": geometry(*geo, **kw), "kernel": kernel, "form": form,
            "splits": splits}


def _tiles():
    return [
        # 64-pixel tiles: P = 65, 77, 99 and channel tiles of 72, 136 (128 + 8), 200 (128 + 72)
        conv("tile:64", IGEMM, 64, 1, 64, 5, 13, 72, 1, stats=True),
        conv("tile:64", IGEMM, 64, 1, 64, 7, 11, 136, 3, pad=1, pad_mode=1, bias=True, stats=True),
        conv("tile:64", IGEMM, 64, 1, 128, 9, 11, 200, 3, pad=1, stats=True),
        # Cout = 1000 / 1024: eight channel tiles, 128-pixel tiles from 32 of them on (P = 3969: the last holds one pixel)
        conv("tile:128", IGEMM, 128, 1, 64, 126, 126, 1000, 2, stride=2, bias=True, stats=True),
        conv("tile:127-tiles", IGEMM, 64, 1, 64, 62, 64, 1024, 1, stats=True),
        # 48 K-steps (>= 40) and P = 8001: 32 256-pixel tiles, the last of 65 pixels; P = 7936: 31 of them, so 128
        conv("tile:256", IGEMM, 256, 1, 192, 66, 130, 1000, 4, bias=True, stats=True),
        conv("tile:255-tiles", IGEMM, 128, 1, 192, 65, 131, 1024, 4, stats=True),
    ]


def _taps():
    out = []
    fixed = ((3, 3), (4, 4), (7, 1), (1, 7), (4, 1), (2, 2), (2, 1), (1, 2), (1, 1))
    for i, (kh, kw) in enumerate(fixed):      # stride 2 on 9 x 11, alternately zero and reflection padding
        out.append(conv(f"taps:{kh}x{kw}", IGEMM, 64, 1 + i % 2, 64, 9, 11, (40, 72, 136)[i % 3], (kh, kw), stride=2,
                        pad=(kh // 2, kw // 2), pad_mode=i % 2, bias=i % 2 == 0, stats=True))
    out.append(conv("taps:runtime", IGEMM, 64, 1, 64, 9, 11, 72, 5, stride=2, pad=2, pad_mode=1, stats=True))
    out.append(conv("taps:runtime", IGEMM, 64, 2, 64, 9, 11, 40, (3, 1), stride=(2, 1), pad=(1, 0), bias=True))
    out.append(conv("taps:runtime", IGEMM, 64, 1, 64, 9, 11, 136, 7, pad=3, pad_mode=1, stats=True))   # IR2RGB_MAX_TAPS
    out.append(conv("thin:4x4", IGEMM, 64, 1, 64, 9, 11, 32, 4, stride=2, pad=1, bias=True, stats=True))
    out.append(conv("thin:33", IGEMM, 64, 1, 64, 9, 11, 33, 4, stride=2, pad=1, bias=True, stats=True))
    out.append(conv("thin:1x7", IGEMM, 64, 2, 64, 5, 9, 3, (1, 7), pad=(0, 3), pad_mode=1, bias=True))
    out.append(conv("thin:1x7", IGEMM, 64, 1, 128, 5, 9, 32, (1, 7), pad=(0, 3), pad_mode=1, stats=True))
    return out


def _epilogue():
    out = []
    for i, Cout in enumerate((3, 5, 130)):    # scalar stores; 130: the second channel tile holds two channels
        out.append(conv("store:scalar", IGEMM, 64, 2, 64, 5, 7, Cout, 3, pad=1, bias=i != 1, stats=i != 0))
    for i, Cout in enumerate((4, 12, 36)):    # 8-byte stores straight from the registers (Cout % 8 != 0)
        out.append(conv("store:vector", IGEMM, 64, 2, 64, 5, 7, Cout, 3, pad=1, pad_mode=1, bias=i != 1, stats=i != 0))
    for Cout in (1, 5, 8, 40):
        out.append(conv("store:f32", IGEMM, 64, 1, 64, 5, 7, Cout, 3, pad=1, out_f32=1, bias=Cout != 8, stats=Cout == 40))
    for act in (1, 2, 3):
        for Cout in (5, 72):
            out.append(conv("act", IGEMM, 64, 1, 64, 5, 7, Cout, 3, pad=1, act=act, bias=True, stats=Cout == 72))
    # tiles cut inside a sample: 77 pixels = 64 + 13 per sample; 1325 = 10 * 128 + 45 per sample at TP = 128
    out.append(conv("stats:per-sample", IGEMM, 64, 3, 64, 7, 11, 72, 3, pad=1, sps=1, stats=True))
    out.append(conv("stats:per-sample", IGEMM, 64, 3, 64, 7, 11, 5, 3, pad=1, sps=1, bias=True, stats=True))
    out.append(conv("stats:per-sample", IGEMM, 128, 3, 64, 25, 53, 1024, 1, sps=1, stats=True))
    return out


def _slices():
    f = dict(entry="fwd")
    return [
        conv("slice:in", IGEMM, 64, 2, 64, 5, 7, 72, 3, pad=1, ldx=136, ci_off=8, bias=True, **f),
        conv("slice:in", IGEMM, 64, 1, 64, 5, 7, 40, 3, pad=1, pad_mode=1, ldx=192, ci_off=64, stats=True, **f),
        conv("slice:out", IGEMM, 64, 2, 64, 5, 7, 72, 3, pad=1, ldy=200, co_off=8, bias=True, stats=True, **f),
        conv("slice:out", IGEMM, 64, 1, 64, 5, 7, 40, 3, pad=1, ldy=172, co_off=100, **f),          # not staged: co_off % 8
        conv("slice:out", IGEMM, 64, 1, 64, 5, 7, 136, 1, ldx=72, ci_off=8, ldy=328, co_off=192, bias=True, **f),
        conv("slice:odd", IGEMM, 64, 2, 64, 5, 7, 3, 3, pad=1, ldy=7, co_off=1, bias=True, **f),
        conv("slice:odd", IGEMM, 64, 1, 64, 5, 7, 5, 3, pad=1, out_f32=1, ldy=9, co_off=3, stats=True, **f),
    ]


def _borders():
    out = []
    for H, W in ((4, 7), (6, 4), (7, 6), (4, 4)):           # 7x7 reflection: pad < H <= 2 * pad
        out.append(conv("border:reflect-deep", IGEMM, 64, 2, 64, H, W, 40, 7, pad=3, pad_mode=1, stats=True))
    out.append(conv("border:reflect-deep", IGEMM, 64, 1, 64, 2, 2, 72, 3, pad=1, pad_mode=1, bias=True))
    out.append(conv("border:one-pixel", IGEMM, 64, 2, 64, 3, 9, 40, 3, stats=True))                   # Hout = 1
    out.append(conv("border:one-pixel", IGEMM, 64, 1, 64, 10, 2, 40, 4, stride=2, pad=1, bias=True))   # Wout = 1
    out.append(conv("border:one-pixel", IGEMM, 64, 1, 64, 1, 1, 72, 1, bias=True, stats=True))
    out.append(conv("border:overpad", IGEMM, 64, 1, 64, 1, 2, 40, 3, pad=2, bias=True, stats=True))
    out.append(conv("border:overpad", IGEMM, 64, 2, 64, 2, 2, 72, 7, pad=3))
    out.append(conv("border:two-samples", IGEMM, 64, 3, 64, 5, 9, 72, 3, pad=1, pad_mode=1, bias=True, stats=True))
    return out


def _classes():
    t = dict(transposed=1, stride=2)
    return [
        # 9 x 13 / 10 x 14 outputs: classes of 35, 30, 28, 24 pixels -- one workgroup each, seven padding blocks behind it
        conv("classes:64", CLASSES, 64, 1, 64, 5, 7, 72, 3, pad=1, bias=True, stats=True, **t),
        conv("classes:64", CLASSES, 64, 2, 64, 5, 7, 136, 3, pad=1, output_padding=1, stats=True, **t),
        conv("classes:64", CLASSES, 64, 1, 128, 5, 3, 40, 4, pad=1, bias=True, act=3, **t),
        conv("classes:64", CLASSES, 64, 2, 64, 5, 7, 72, 3, pad=1, output_padding=(0, 1), out_f32=1, **t),
        conv("classes:two", CLASSES, 64, 1, 64, 5, 7, 72, (4, 1), transposed=1, stride=(2, 1), pad=(1, 0), bias=True, stats=True),
        conv("classes:1x1-input", CLASSES, 64, 1, 64, 1, 1, 72, 3, pad=1, output_padding=1, bias=True, stats=True, **t),
        conv("classes:1x1-input", IGEMM, 64, 1, 64, 1, 1, 72, 3, pad=1, bias=True, **t),      # one output pixel: one class
        conv("classes:thin", CLASSES, 64, 2, 64, 5, 7, 3, 3, pad=1, output_padding=1, bias=True, **t),
        conv("classes:thin", CLASSES, 64, 1, 64, 5, 7, 32, 4, pad=1, stats=True, **t),
        # Cout = 1024: 65 x 65 -> 34 * 8 = 272 workgroups of 128 pixels (<= 320: 64); 71 x 73 -> 41 * 8 = 328 (128)
        conv("classes:64-capped", CLASSES, 64, 1, 64, 33, 33, 1024, 3, pad=1, stats=True, **t),
        conv("classes:128", CLASSES, 128, 1, 64, 36, 37, 1024, 3, pad=1, bias=True, stats=True, **t),
        conv("transposed:one-class", IGEMM, 64, 2, 64, 5, 7, 72, 3, transposed=1, pad=1, bias=True, stats=True),
        conv("transposed:one-class", IGEMM, 64, 1, 64, 5, 7, 40, 4, transposed=1, pad=1),
    ]


def _dots():
    f = dict(out_f32=1)
    return [
        conv("dot", DOT, 64, 1, 512, 1, 1, 1, 1, bias=True, **f),                           # P = 1
        conv("dot", DOT, 64, 1, 1024, 1, 3, 1, 1, **f),                                     # P = 3
        conv("dot", DOT, 64, 1, 1024, 2, 6, 1, 4, pad=1, bias=True, act=1, **f),            # P = 5
        conv("dot", DOT, 64, 2, 512, 2, 2, 1, 4, pad=2, bias=True, **f),                    # P = 18
        conv("dot:capped", DOT, 64, 1, 512, 55, 149, 1, 1, bias=True, **f),                # P = 8195 > 8192 waves
        conv("dot:capped", DOT, 64, 1, 512, 56, 150, 1, 4, pad=1, **f),
        conv("dot:slice", DOT, 64, 2, 512, 3, 3, 1, 4, pad=2, ldx=520, ci_off=8, bias=True, entry="fwd", **f),
        conv("dot:stats", IGEMM, 64, 1, 1024, 2, 6, 1, 4, pad=1, bias=True, act=1, stats=True, named=DOT, **f),
        conv("dot:stats", IGEMM, 64, 1, 512, 1, 3, 1, 1, stats=True, named=DOT, **f),
    ]


def _patches():
    s = dict(bias=True, stats=True)
    return [
        # variant 1 (2 x 64 pixels x 64 channels): 2 * 12 * 3 * 3 = 216 tiles, Hout = 23 odd, Wout = 190 = 2 * 64 + 62
        conv("patch:1", PATCH, (2, 64), 2, 256, 23, 190, 192, 3, pad=1, pad_mode=1, **s),
        conv("patch:1", PATCH, (2, 64), 2, 256, 25, 192, 192, 3, pad=0, stats=True),
        conv("patch:1", PATCH, (2, 64), 2, 256, 21, 188, 192, 3, pad=2, bias=True),
        conv("patch:adjoint", PATCH, (2, 64), 2, 128, 24, 192, 192, 3, pad=1, pad_mode=2, **s),
        # Cout = 128, Wout = 250: 25 * 4 * 2 = 200 tiles at Hout = 50
        conv("patch:200-tiles", PATCH, (2, 64), 1, 256, 50, 250, 128, 3, pad=1, **s),
        # Cout = 64, Wout = 64: one tile per row pair -- 200 at Hout = 399, 199 at Hout = 397 (the general kernel)
        conv("patch:200-tiles", PATCH, (2, 64), 1, 256, 399, 64, 64, 3, pad=1, pad_mode=1, stats=True),
        conv("patch:199-tiles", IGEMM, 64, 1, 256, 397, 64, 64, 3, pad=1, pad_mode=1, **s),
        # variant 2 (2 x 128 x 128): 25 * 1 * 8 = 200 tiles
        conv("patch:2", PATCH, (2, 128), 1, 256, 49, 120, 1024, 3, pad=1, pad_mode=1, **s),
        conv("patch:adjoint", PATCH, (2, 128), 1, 128, 50, 128, 1024, 3, pad=1, pad_mode=2, stats=True),
        # ... without padding, and with two reflected pixels on each side of the 2 x 128 tile
        conv("patch:2", PATCH, (2, 128), 1, 256, 51, 122, 1024, 3, pad=0, stats=True),
        conv("patch:2", PATCH, (2, 128), 1, 256, 47, 118, 1024, 3, pad=2, pad_mode=1, **s),
        # the split forms (Cin >= 512, a workspace): variant 4 (4 rows) at Hout = 11, variant 3 at Hout = 10 (12 / 10 > 1.13)
        conv("patch:4", PATCH, (2, 64), 3, 512, 11, 64, 768, 3, pad=1, workspace=True, **s),
        conv("patch:3", PATCH, (2, 64), 3, 512, 10, 64, 1024, 3, pad=1, pad_mode=1, workspace=True, **s),
        # ... both at padding 0 and 2 (Hout = 11 / 10 again), the latter reflected two pixels deep
        conv("patch:4", PATCH, (2, 64), 3, 512, 13, 66, 768, 3, pad=0, workspace=True, stats=True),
        conv("patch:4", PATCH, (2, 64), 3, 512, 9, 62, 768, 3, pad=2, pad_mode=1, workspace=True, **s),
        conv("patch:3", PATCH, (2, 64), 3, 512, 12, 66, 1024, 3, pad=0, workspace=True, bias=True),
        conv("patch:3", PATCH, (2, 64), 3, 512, 8, 62, 1024, 3, pad=2, pad_mode=1, workspace=True, **s),
        conv("patch:3", PATCH, (2, 64), 3, 512, 8, 62, 1024, 3, pad=2, workspace=True, stats=True),
    ]


def _thin1x7():
    k = dict(k=(1, 7), pad=(0, 3), pad_mode=1, out_f32=1)
    out = []
    for i, W in enumerate((4, 5, 127, 129)):
        Cin, Cout = (64, 128)[i % 2], (4, 8, 32, 4)[i]
        out.append(conv("thin1x7", THIN7, 64, 1 + i % 2, Cin, 3, W, Cout, **k))
    # (the plan wants 16-byte pixel rows, ldy % 4 == 0: one or three channels only inside a wider buffer)
    out.append(conv("thin1x7:slice", THIN7, 64, 1, 64, 3, 4, 1, ldy=4, entry="fwd", **k))
    out.append(conv("thin1x7", THIN7, 64, 1, 64, 2, 9, 32, **k))
    out.append(conv("thin1x7:slice", THIN7, 64, 2, 128, 3, 9, 3, ldy=4, entry="fwd", **k))
    out.append(conv("thin1x7:slice", THIN7, 64, 1, 64, 3, 5, 4, ldx=72, ci_off=8, ldy=12, co_off=8, entry="fwd", **k))
    # 257 * 2 = 514 segments on 512 workgroups; its general-kernel plan (the statistics rows) has 260 tiles of 128
    out.append(conv("thin1x7:wrap", THIN7, 128, 1, 64, 257, 129, 4, **k))
    out.append(conv("thin1x7:bias", IGEMM, 64, 1, 64, 3, 5, 4, bias=True, named=THIN7, **k))
    out.append(conv("thin1x7:bias", IGEMM, 64, 2, 128, 3, 127, 32, stats=True, named=THIN7, **k))
    return out


def _col7x1():
    k = dict(k=(7, 1), pad=(3, 0), pad_mode=1)
    out = []
    i = 0
    for H in (4, 7, 9):
        for W in (1, 31, 33):
            out.append(conv("col7x1", COL7, (8, 32), 1 + i % 2, 64, H, W, (64, 128)[i % 2], bias=i % 3 == 0,
                            stats=i % 4 != 3, **k))
            i += 1
    out.append(conv("col7x1", COL7, (8, 32), 2, 64, 9, 33, 128, ldx=72, ci_off=8, ldy=132, co_off=4, entry="fwd", bias=True, **k))
    out.append(conv("col7x1:wrap", COL7, (8, 32), 3, 64, 44, 929, 64, bias=True, stats=True, **k))   # 3 * 6 * 30 = 540 tiles
    return out


EDGE_CONV = (_tiles() + _taps() + _epilogue() + _slices() + _borders() + _classes() + _dots() + _patches() + _thin1x7()
             + _col7x1())

ONETAP, NINE, LINE, COL = "conv_wgrad_kernel", "conv_wgrad3x3_kernel", "conv_wgrad_line_kernel", "conv_wgrad_col_kernel"


def _onetap():
    out = []
    # 3x3 with Cb = 64: tap pairs (five, the last half-empty); Cb = 72: one tap per workgroup.  Q = 35 < 64, 99, 231
    out.append(wgrad("onetap:tpb2", ONETAP, 1, 1, 64, 5, 7, 72, 3, pad=1))
    out.append(wgrad("onetap:tpb2", ONETAP, 1, 3, 8, 7, 11, 8, 3, pad=1, pad_mode=1))
    out.append(wgrad("onetap:tpb2", ONETAP, 1, 1, 24, 9, 11, 200, (4, 1), pad=(1, 0)))
    for Cin, Cout in ((72, 24), (136, 200), (200, 136), (72, 8)):
        out.append(wgrad("onetap:tpb1", ONETAP, 1, 1, Cin, 9, 11, Cout, 3, pad=1, pad_mode=int(Cin == 72)))
    out.append(wgrad("onetap:tpb1", ONETAP, 1, 2, 8, 5, 7, 8, 1))
    # Q = 4096 (64 K-steps), one tile, 64 elements: sixteen splits of four K-steps cost least; at Q = 448 (seven) none is allowed
    out.append(wgrad("onetap:split", ONETAP, 16, 1, 8, 64, 64, 8, 1))
    out.append(wgrad("onetap:split", ONETAP, 8, 2, 72, 33, 31, 24, 3, pad=1))
    out.append(wgrad("onetap:stride2", ONETAP, 1, 1, 72, 9, 11, 24, 3, stride=2, pad=1))
    out.append(wgrad("onetap:stride2", ONETAP, 1, 3, 64, 9, 11, 72, 4, stride=2, pad=1))
    out.append(wgrad("onetap:stride2", ONETAP, 1, 2, 128, 17, 9, 128, 3, stride=2, pad=1))
    for op in (0, 1):
        out.append(wgrad("onetap:transposed", ONETAP, 1, 2, 72, 5, 7, 24, 3, transposed=1, stride=2, pad=1, output_padding=op))
    out.append(wgrad("onetap:transposed", ONETAP, 1, 1, 64, 5, 7, 136, 4, transposed=1, stride=2, pad=1))
    out.append(wgrad("onetap:reflect-deep", ONETAP, 1, 2, 24, 3, 4, 8, 5, pad=2, pad_mode=1))          # 25 taps
    out.append(wgrad("onetap:gather-finish", ONETAP, 1, 1, 8, 4, 6, 8, 7, pad=3, pad_mode=1))          # 49 > WF_MAX_TAPS
    out.append(wgrad("onetap:gather-finish", ONETAP, 1, 2, 72, 7, 5, 24, 5, pad=2))
    return out


def _nine():
    return [
        wgrad("nine:direct", NINE, 0, 1, 64, 2, 64, 64, 3, pad=1, pad_mode=1),          # H = 2: every row a border row
        wgrad("nine:direct", NINE, 0, 1, 128, 3, 128, 192, 3, pad=1),                   # Q / 64 = 6 < 16
        wgrad("nine:direct", NINE, 0, 2, 64, 3, 64, 128, 3, pad=1, pad_mode=1),
        wgrad("nine:split", NINE, 3, 2, 128, 5, 192, 192, 3, pad=1, pad_mode=1),        # 30 K-steps: three splits of ten
        wgrad("nine:split", NINE, 2, 1, 64, 9, 128, 64, 3, pad=1),                      # 18 K-steps: two of nine
    ]


def _lines():
    return [
        # 7x1: W = 70 is a whole segment and one of six pixels; 18 K-steps in two splits
        wgrad("line:col7", COL, 2, 1, 64, 9, 70, 64, (7, 1), pad=(3, 0), pad_mode=1),
        wgrad("line:line7", LINE, 1, 2, 64, 9, 5, 128, (7, 1), stride=(2, 1), pad=(3, 0), pad_mode=1),
        wgrad("line:col4", COL, 1, 1, 128, 10, 7, 64, (4, 1), stride=(2, 1), pad=(1, 0)),
        wgrad("line:line4", LINE, 2, 2, 64, 9, 5, 64, (4, 1), pad=(1, 0)),
        wgrad("line:1x7", LINE, 1, 1, 64, 5, 5, 64, (1, 7), pad=(0, 3), pad_mode=1),    # pad < W <= 2 * pad
        wgrad("line:1x7", LINE, 4, 2, 128, 9, 70, 64, (1, 7), pad=(0, 3)),           # 36 K-steps, two tiles: four of nine
        wgrad("line:one-split", COL, 1, 1, 64, 3, 5, 64, (7, 1), pad=(3, 0)),           # three K-steps
        wgrad("line:short-last-split", COL, 2, 1, 64, 19, 5, 64, (7, 1), pad=(3, 0)),   # 19 K-steps: ten and nine
        wgrad("line:wide-finish", COL, 65, 1, 64, 130, 200, 64, (7, 1), pad=(3, 0), pad_mode=1),   # 520 K-steps of 8
        wgrad("line:reflect-deep", COL, 1, 2, 64, 4, 5, 64, (7, 1), pad=(3, 0), pad_mode=1),
        wgrad("line:reflect-deep", COL, 1, 1, 64, 6, 9, 128, (7, 1), pad=(3, 0), pad_mode=1),
        # 3x3 / stride 2: tl = (Cout / 64) * (Cin / 64) of 1, 2 and 128 take the line kernel, 4 the one-tap kernel
        wgrad("line:3x3s2", LINE, 1, 1, 64, 9, 11, 64, 3, stride=2, pad=1),
        wgrad("line:3x3s2", LINE, 1, 2, 64, 10, 7, 128, 3, stride=2, pad=1),
        wgrad("line:3x3s2", LINE, 1, 1, 512, 17, 9, 1024, 3, stride=2, pad=1),
        wgrad("line:3x3s2-transposed", LINE, 1, 1, 1024, 9, 5, 512, 3, transposed=1, stride=2, pad=1, output_padding=1),
        wgrad("line:3x3s2-transposed", LINE, 1, 2, 64, 5, 7, 64, 3, transposed=1, stride=2, pad=1),
        wgrad("onetap:tl4", ONETAP, 1, 1, 128, 9, 11, 128, 3, stride=2, pad=1),
    ]


EDGE_WGRAD = _onetap() + _nine() + _lines()


# ---------------------------------------------------------------------------------------------------------------------
# EDGE_RANGE: the records of tests/test_range_cpu.py and tests/test_range_gpu.py, each with the modes that apply
# (oracle/range_cases.py: "overflow" O, "subnormal" U, "nonfinite" N).  The smallest EDGE record of each form is
# reused; ``plant`` = (operand, position, value) of the nonfinite mode.
#
#   record                                   modes   half store / fp32 consumer reached
#   conv store:scalar (Cout 5)               O U N   conv_igemm_body epilogue, scalar Half<>::cvt stores (conv_mfma.hip)
#   conv store:vector (Cout 36)              O U N   ... 8-byte stores from the registers
#   conv tile:64 (Cout 72), tile:128         O U N   ... the staged epilogue (LDS, 16-byte stores), 64- and 128-pixel tiles
#   conv thin:4x4 (Cout 32)                  O U N   ... the THIN tile's stores
#   conv act (bias, LeakyReLU 0.2, Cout 72)  O U N   ... bias and activation before the store
#   conv classes:two, transposed:one-class   O U N   conv_igemm_classes_kernel's stores; a transposed single class
#   conv patch:1, patch:adjoint (pad_mode 2) O U N   conv3x3_patch.hip stores, the reflect-adjoint fold
#   conv col7x1                              O U N   conv7x1_col.hip stores
#   conv dot, thin1x7 (fp32 outputs)           U N   conv_dot_kernel / conv1x7_thin.hip: fp32 consumers of half operands
#   wgrad nine:direct / nine:split,            U N   wgrad_mfma.hip: fp32 consumers of the half gradient, plain and
#     line:col7 / line:line7, onetap:split             accumulating (ir2rgb_conv2d_wgrad_acc); plants in gy and in x
#   bn_bwd 4096 / 4097 / 2049 pixels         O U N   backward.hip f2h of gy (one launch, two passes, C = 2048), act 0 / 1 / 2,
#     (+ act | 16, + bias-only)                        dgamma / dbeta; plants in gz and in y
#   bn_apply, bn_finalize_apply              O   N   pointwise.hip f2h of the two apply kernels; plants in x and in a
#                                                      statistics row
#   bn_finalize_ex (32- and 8-channel forms)     N   the same statistics-row plant through the two-launch path
#   the three layout converters              O U N   pointwise.hip f2h of nchw_to_nhwc[_slice]_kernel, h2f of the inverse
#   head_finish_bwd (dT, dbias)              O U N   heads.hip:112, the (_Float16) cast of head_finish_bwd_kernel
#   flow_upsample_slice                      O U N   heads.hip:310, the (_Float16) casts of flow_up_kernel
#   thin_grad_expand (g8, g64, dbias)        O U N   backward.hip f2h of the expanded logit gradient
#   fold_reflect                               U N   backward.hip f2h of the folded gradient (sums of <= 4 inputs)
#   xexpand                                  O U N   pointwise.hip:377 f2h of xexpand_kernel
#   xexpand_bwd                                U N   its adjoint: an fp32 consumer of the half gradient
#   correlation_nhwc_half, out mode 1        O   N   correlation_mfma.hip's half store behind the LeakyReLU
#   loss_multi_bwd                           O U N   losses.hip:127 f2h(gout * weight / n), the root of the scaled backward
def _of(recs, form=None, **fields):
    for r in recs:
        where = r.get("desc") or {}
        if (form is None or r.get("form") == form) and r.get("entry", "fwd_ws") != "fwd" and \
                all(where.get(k, r.get(k)) == v for k, v in fields.items()):
            return r
    raise LookupError((form, fields))


def ranged(rec, modes, plant=None, **kw):
    rec = dict(rec, modes=tuple(modes), **kw)
    if plant is not None:
        rec["plant"] = tuple(plant)
    return rec


O_U_N, U_N, O_N = ("overflow", "subnormal", "nonfinite"), ("subnormal", "nonfinite"), ("overflow", "nonfinite")
_PLANTS = (("x", "first", "nan"), ("x", "last", "+inf"), ("x", "border", "-inf"), ("w", "first", "+inf"),
           ("x", "border", "nan"), ("x", "last", "-inf"))


def _range_convs():
    half = [_of(EDGE_CONV, "store:scalar", Cout=5), _of(EDGE_CONV, "store:vector", Cout=36), _of(EDGE_CONV, "tile:64", Cout=72),
            _of(EDGE_CONV, "tile:128"), _of(EDGE_CONV, "thin:4x4"), _of(EDGE_CONV, "act", Cout=72, act=1),
            _of(EDGE_CONV, "classes:two"), _of(EDGE_CONV, "transposed:one-class"), _of(EDGE_CONV, "patch:1"),
            _of(EDGE_CONV, "patch:adjoint"), _of(EDGE_CONV, "col7x1", Win=31)]
    f32 = [_of(EDGE_CONV, "dot", N=2), _of(EDGE_CONV, "thin1x7", Win=5)]
    out = [ranged(r, O_U_N, _PLANTS[i % len(_PLANTS)]) for i, r in enumerate(half)]
    out += [ranged(r, U_N, _PLANTS[i]) for i, r in enumerate(f32)]
    out.append(ranged(_of(EDGE_CONV, "act", Cout=72, act=1), ("nonfinite",), ("bias", "last", "nan")))
    return out


def _range_wgrads():
    recs = [_of(EDGE_WGRAD, "nine:direct", N=2), _of(EDGE_WGRAD, "nine:split", N=1), _of(EDGE_WGRAD, "line:col7"),
            _of(EDGE_WGRAD, "line:line7"), _of(EDGE_WGRAD, "onetap:split", Cin=72)]
    vals = ("nan", "+inf", "-inf")
    out = []
    for i, r in enumerate(recs):
        out.append(ranged(r, U_N, ("gy", ("first", "last")[i % 2], vals[i % 3])))
        out.append(ranged(r, ("nonfinite",), ("x", ("last", "border", "first")[i % 3], vals[(i + 1) % 3])))
    return out


def _range_bns():
    out = []
    vals = ("nan", "+inf", "-inf")
    for i, (npix, C) in enumerate(((4096, 64), (4097, 128), (2049, 2048))):
        for act in (0, 1, 2):
            j = 3 * i + act
            out.append(ranged(bwd(npix, C, act), O_U_N, ("gz", ("first", "last")[j % 2], vals[j % 3])))
            if act != 1:
                out.append(ranged(bwd(npix, C, act), ("nonfinite",), ("y", ("last", "first")[j % 2], vals[(j + 1) % 3])))
    out.append(ranged(bwd(4097, 64, 2 | 16), O_U_N, ("gz", "last", "+inf")))
    out.append(ranged(bwd(4096, 128, 1 | 16), O_U_N, ("gz", "first", "nan")))
    out.append(ranged(bwd(513, 64, 1, scale=False), U_N, ("gz", "last", "-inf")))
    out.append(ranged(bwd(4097, 512, 2, scale=False), U_N, ("gz", "first", "nan")))
    for i, (npix, C, res, act) in enumerate(((257, 64, 0, 1), (257, 24, 1, 2), (3, 8, 2, 0))):
        out.append(ranged(apply(npix, C, res, act), O_N, ("x", ("last", "first")[i % 2], vals[i % 3])))
    for i, (rows, C, npix, res, act) in enumerate(((9, 64, 129, 0, 1), (2, 192, 33, 1, 2), (128, 64, 1000, 2, 0))):
        r = finalize_apply(rows, C, npix, res, act)
        r.pop("two_launch")
        out.append(ranged(r, O_N, ("x", ("first", "last")[i % 2], vals[(i + 1) % 3])))
        out.append(ranged(r, ("nonfinite",), ("rows", "last", "nan")))
    out.append(ranged(finalize(9, 72, 129, upd=2), ("nonfinite",), ("rows", "last", "nan")))
    out.append(ranged(finalize(2049, 64, 4100, bias=False), ("nonfinite",), ("rows", "last", "nan")))
    return out


def _range_converters():
    out = []
    for e in ("ir2rgb_nchw_f32_to_nhwc_half", "ir2rgb_nhwc_half_to_nchw_f32"):
        for (H, W), C in (((5, 13), 65), ((3, 43), 3)):
            out.append(ranged(op(e, N=2, C=C, H=H, W=W, dtype=1), O_U_N if e.endswith("half") else U_N))
    for act in (0, 2):
        out.append(ranged(op("ir2rgb_nchw_f32_to_nhwc_half_slice", N=2, C=65, H=5, W=13, ld=75, c_off=3, act=act, dtype=1),
                          O_U_N))
    return out


# loss_multi_bwd: three L1 items (half operands) whose weight / n puts gout * weight / n on both sides of 65520 at
# gout = 2^23 * (1, 2, .5, 4) (81920 and 158875 against 5110) and into [2^-21, 2^-15) at 2^-10 * the same; an MSE and a
# masked-L1 item (fp32 gradients) beside them.  The nonfinite plant names the slot of gout.
RANGE_LOSS = [_item(0, 2048, 1, 10.0), _item(0, 4104, 2, 5.0), _item(0, 264, 0, 5.0), _item(1, 257, 1, 1.0, 1.0),
              _item(2, 135, 3, 10.0, hw=15, chw=45)]


def _range_ops():
    e = lambda entry, **want: next(r for r in EDGE if r["entry"] == entry and  # noqa: E731
                                   all(dict(zip(ARGS[entry].split(), r["args"]))[k] == v for k, v in want.items()))
    loss = {"kind": "op", "entry": "ir2rgb_loss_multi_bwd", "count": len(RANGE_LOSS), "dtype": 1, "items": RANGE_LOSS}
    return [
        ranged(e("ir2rgb_head_finish_bwd", H=9, W=5, Cout=3), O_U_N, ("gout", "last", "nan")),
        ranged(e("ir2rgb_head_finish_bwd", H=4, W=5, Cout=8), O_U_N, ("gout", "first", "-inf")),
        ranged(e("ir2rgb_thin_grad_expand", Cout=5), O_U_N, ("gz", "last", "+inf")),
        ranged(e("ir2rgb_thin_grad_expand", Cout=8), O_U_N, ("gz", "first", "nan")),
        ranged(e("ir2rgb_fold_reflect", H=4, C=64), U_N, ("dxpad", "first", "nan")),
        ranged(e("ir2rgb_fold_reflect", H=5, C=72), U_N, ("dxpad", "last", "-inf")),
        ranged(e("ir2rgb_xexpand_bwd", Cin=9, W=4), U_N, ("dxe", "first", "+inf")),
        ranged(e("ir2rgb_xexpand_bwd", Cin=13, W=254), U_N, ("dxe", (1, 2, 64, 51), "nan")),    # the last used channel
        ranged(e("ir2rgb_xexpand", Cin=9, W=129), O_U_N, ("x", "border", "nan")),
        ranged(e("ir2rgb_xexpand", Cin=13, W=5), O_U_N, ("x", "last", "-inf")),
        ranged(e("ir2rgb_flow_upsample_slice", h=3, w=5, bias=True), O_U_N, ("x", "last", "+inf")),
        ranged(e("ir2rgb_flow_upsample_slice", h=1, w=9, bias=False), O_U_N, ("x", "first", "nan")),
        # (21 x 33 pixels: a third of the 441 displacements stay inside the image, so that the overflow mode is live)
        ranged(flow("ir2rgb_correlation_nhwc_half", "mfma:kc4", lda=128, offa=0, ldb=128, offb=0, out_mode=1, ldo=512, offo=32,
                    slope=0.1, N=1, C=128, H=21, W=33, dtype=1), O_N, ("f1", "first", "nan")),
        ranged(flow("ir2rgb_correlation_nhwc_half", "mfma:kc8", lda=256, offa=0, ldb=320, offb=64, out_mode=1, ldo=448, offo=7,
                    slope=0.1, N=2, C=256, H=21, W=31, dtype=1), O_N, ("f1", "last", "-inf")),
        ranged(loss, O_U_N, ("gout", 1, "nan"), ek=(23, 10)),
        ranged(loss, ("nonfinite",), ("gout", 2, "-inf"), ek=(23, 10)),
        ranged(loss, ("nonfinite",), ("gout", 0, "+inf"), ek=(23, 10)),
    ]


EDGE_RANGE = _range_convs() + _range_wgrads() + _range_bns() + _range_converters() + _range_ops()
RANGE_CASES = [(r, m) for r in EDGE_RANGE for m in r["modes"]]
