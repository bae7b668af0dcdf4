"""The EDGE_CONV / EDGE_WGRAD records of oracle/edge_records.py, checked without a GPU.

* Every form named in CONV_FORMS / WGRAD_FORMS has a record.
* The built library's host-only queries agree with what the records state by hand: the kernel's name, whether the
  launch wants a workspace, the statistics rows that the stated tile implies, the weight gradient's split count.
  The queries cannot tell the line / column kernels from the one-tap kernel at an equal split count (both report
  splits * taps * Ca * Cb workspace elements), nor the forms of one kernel from each other: there the record's ``form``
  -- and, for every weight-gradient record, its ``kernel`` -- is documentation of what the GPU replay exercises, not
  something this file can hold the library to.
* oracle/conv_ref.py (im2col) agrees with torch's own fp64 convolutions and with autograd at these shapes.
* oracle/bounds.py rejects a dropped tap, a shifted tile and a lost split at these shapes.
"""
import pytest
import torch
import torch.nn.functional as F

from oracle import bounds as B
from oracle import conv_ref as R
from oracle import replay
from oracle import window as WG
from oracle import edge_records as ER
from oracle.edge_records import CONV_FORMS, EDGE_CONV, EDGE_WGRAD, WGRAD_FORMS
from test_kernel_bounds_cpu import _operands, _rejected, _rounded

SMALL_FLOP = 1e9


@pytest.fixture(scope="module")
def lib():
    from ir2rgb_amd import _lib, build
    build.build()
    return _lib.lib()


def _desc(d):
    from ir2rgb_amd import conv as C
    from ir2rgb_amd._lib import ConvDesc
    return C.sealed(ConvDesc(*[d[f] for f in WG.DESC_FIELDS]))


def _flop(d):
    return 2.0 * d["N"] * d["Hout"] * d["Wout"] * d["Cout"] * d["Cin"] * d["kh"] * d["kw"]


def test_every_form_has_a_record():
    assert {r["form"] for r in EDGE_CONV} == set(CONV_FORMS)
    assert {r["form"] for r in EDGE_WGRAD} == set(WGRAD_FORMS)
    assert len(set(CONV_FORMS)) == len(CONV_FORMS) and len(set(WGRAD_FORMS)) == len(WGRAD_FORMS)


def test_no_reference_is_larger_than_60_gflop():
    assert max(_flop(r["desc"]) for r in EDGE_CONV + EDGE_WGRAD) <= 60e9


def implied_rows(rec):
    """Statistics rows that the record's stated tile implies."""
    d, tile = rec["desc"], rec["tile"]
    n, ho, wo = d["N"], d["Hout"], d["Wout"]
    if isinstance(tile, tuple):
        th, tw = tile
        if rec["kernel"] == ER.PATCH:
            return n * -(-ho // th) * -(-wo // tw)
        assert rec["kernel"] == ER.COL7
        return n * -(-ho // th) * -(-wo // tw) * (2 if d["Cout"] == 64 else 1)     # one row per pixel half at 64 channels
    if d["transposed"]:             # one tile sequence per sub-pixel class
        sh, sw = d["stride_h"], d["stride_w"]
        return sum(-(-(n * len(range(a, ho, sh)) * len(range(b, wo, sw))) // tile)
                   for a in range(sh) for b in range(sw) if a < ho and b < wo)
    if d["stats_per_sample"]:
        return n * -(-(ho * wo) // tile)
    return -(-(n * ho * wo) // tile)


@pytest.mark.parametrize("rec", EDGE_CONV, ids=replay.ids(EDGE_CONV))
def test_library_agrees_with_the_forward_record(lib, rec):
    from ir2rgb_amd import conv as C
    desc = _desc(rec["desc"])
    assert C.kernel_name(desc) == rec.get("named", rec["kernel"])
    if "named" in rec:              # the launch leaves the named kernel only through an argument the query cannot see
        assert rec["named"] in (ER.DOT, ER.THIN7) and rec["kernel"] == ER.IGEMM
        assert rec["stats"] or (rec["named"] == ER.THIN7 and rec["bias"])
    assert (lib.ir2rgb_conv2d_fwd_workspace_bytes(desc) > 0) == rec["workspace"]
    assert lib.ir2rgb_conv2d_stats_rows(desc) == implied_rows(rec)


@pytest.mark.parametrize("rec", EDGE_WGRAD, ids=replay.ids(EDGE_WGRAD))
def test_library_agrees_with_the_wgrad_record(lib, rec):
    d = rec["desc"]
    elems = d["kh"] * d["kw"] * d["Cin"] * d["Cout"]
    ws = lib.ir2rgb_conv2d_wgrad_workspace_elems(_desc(d))
    assert ws > 0
    assert ws // elems == rec["splits"] and (ws % elems == 0 or rec["splits"] == 0)
    # the accumulating call never takes the nine-tap kernel: its workspace is the one-tap kernel's slabs
    acc = lib.ir2rgb_conv2d_wgrad_acc_workspace_elems(_desc(d))
    assert acc % elems == 0 and acc >= elems
    if rec["kernel"] != ER.NINE:
        assert acc == ws


# ---------------------------------------------------------------------------------------------------------------------
# The references.  Both sides are fp64 sums of the same K (+ bias) products in different orders: each is within
# gamma_K = K * 2^-53 of the exact value relative to S (the sum of the products' magnitudes), so they differ by at most
# 2 * gamma_(K + 2) * S.  The activations are 1-Lipschitz and the weight gradient's K is the pixel count.
def _agree(got, ref, S, K):
    tol = 2.0 * (K + 2) * 2.0 ** -53 * S + 1e-300
    assert got.shape == ref.shape
    assert bool((torch.abs(got - ref) <= tol).all()), float((torch.abs(got - ref) / tol).max())


def _geometry_key(d, fields):
    return tuple(d[f] for f in fields)


FWD_FIELDS = ("N", "Hin", "Win", "Cin", "Hout", "Wout", "Cout", "kh", "kw", "stride_h", "stride_w", "pad_h", "pad_w",
              "pad_mode", "transposed", "act")
# (no pad_mode-2 record is small -- the patch kernel wants 200 tiles -- so one small adjoint geometry is added here)
FWD_GEOS = list({_geometry_key(r["desc"], FWD_FIELDS): (r["desc"], r["bias"]) for r in EDGE_CONV
                 if _flop(r["desc"]) < SMALL_FLOP}.values()) + \
    [(ER.geometry(2, 8, 4, 6, 16, 3, pad=1, pad_mode=2), True), (ER.geometry(1, 16, 6, 64, 8, 3, pad=1, pad_mode=2), False)]
WG_GEOS = list({_geometry_key(r["desc"], FWD_FIELDS[:-1]): r["desc"] for r in EDGE_WGRAD
                if _flop(r["desc"]) < SMALL_FLOP}.values())


def _torch_forward(d, x, w, bias):
    """torch's own fp64 convolution of the launch, NCHW."""
    x, w = x.double(), w.double()
    b = bias.double() if bias is not None else None
    s, p = (d["stride_h"], d["stride_w"]), (d["pad_h"], d["pad_w"])
    if d["pad_mode"] == 2:          # the gradient of sum(conv(reflect_pad(u), w) * x) with respect to u
        u = torch.zeros(d["N"], d["Cout"], d["Hout"], d["Wout"], dtype=torch.float64, requires_grad=True)
        F.conv2d(F.pad(u, (1, 1, 1, 1), mode="reflect"), w).backward(x)
        y = u.grad
        y = y + b.view(1, -1, 1, 1) if b is not None else y
    elif d["transposed"]:
        op = (d["Hout"] - ((d["Hin"] - 1) * s[0] - 2 * p[0] + d["kh"]), d["Wout"] - ((d["Win"] - 1) * s[1] - 2 * p[1] + d["kw"]))
        y = F.conv_transpose2d(x, w, b, stride=s, padding=p, output_padding=op)
    elif d["pad_mode"] == 1:
        y = F.conv2d(F.pad(x, (p[1], p[1], p[0], p[0]), mode="reflect"), w, b, stride=s)
    else:
        y = F.conv2d(x, w, b, stride=s, padding=p)
    return R.act_fn(d["act"])(y)


@pytest.mark.parametrize("d,bias", FWD_GEOS, ids=[WG.launch_id({"kind": "conv", "entry": "fwd", "desc": g}) for g, _ in FWD_GEOS])
def test_forward_reference_against_torch_fp64(d, bias):
    x, w = _operands(d, 7)
    b = R.draw((d["Cout"],), torch.Generator().manual_seed(8)) if bias else None
    ref, S = R.forward(d, x, w, b)
    got = _torch_forward(d, x, w, b).permute(0, 2, 3, 1)
    _agree(got, ref, S, d["Cin"] * d["kh"] * d["kw"])


@pytest.mark.parametrize("d", WG_GEOS, ids=[WG.launch_id({"kind": "conv", "entry": "wgrad", "desc": g}) for g in WG_GEOS])
def test_wgrad_reference_against_autograd_fp64(d):
    g = torch.Generator().manual_seed(9)
    x = R.draw((d["N"], d["Cin"], d["Hin"], d["Win"]), g)
    gy = R.draw((d["N"], d["Cout"], d["Hout"], d["Wout"]), g)
    ref, S = R.wgrad(d, x, gy)
    w = torch.zeros(R.weight_shape(d), dtype=torch.float64, requires_grad=True)
    _torch_forward(dict(d, act=0), x, w, None).backward(gy.double())
    _agree(w.grad, ref, S, d["N"] * d["Hout"] * d["Wout"])


# ---------------------------------------------------------------------------------------------------------------------
# The bounds at these shapes (the helpers of tests/test_kernel_bounds_cpu.py)
def _record(recs, form, i=0):
    return [r for r in recs if r["form"] == form][i]


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_dropped_tap_at_a_reflected_border_pixel_rejected(fmt):
    """The thin 1x7 record (3 channels, 5 x 9): the first tap of output pixel (0, 0), a reflected one, left out."""
    d = _record(EDGE_CONV, "thin:1x7")["desc"]
    assert d["Cout"] == 3 and d["pad_mode"] == 1
    x, w = _operands(d, 12)
    ref, S = R.forward(d, x, w)
    xp, weff, _, _ = R.effective(d, x, w)
    got = ref.clone()
    got[0, 0, 0] -= weff[:, :, 0, 0].double() @ xp[0, :, 0, 0].double()
    assert not _rejected(_rounded(ref, fmt), ref, S, fmt, B.chain_fwd(d))
    assert _rejected(_rounded(got, fmt), ref, S, fmt, B.chain_fwd(d))


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_shifted_ragged_last_tile_rejected(fmt):
    """The 77-pixel, 136-channel record: the last 64-pixel tile (13 pixels) written one pixel late."""
    rec = _record(EDGE_CONV, "tile:64", 1)
    d, tp = rec["desc"], rec["tile"]
    P = d["N"] * d["Hout"] * d["Wout"]
    start = (P - 1) // tp * tp
    assert start + 1 < P and P % tp
    x, w = _operands(d, 13)
    ref, S = R.forward(d, x, w)
    got = ref.clone()
    got.view(-1, d["Cout"])[start + 1:] = ref.view(-1, d["Cout"])[start:P - 1]
    assert not _rejected(_rounded(ref, fmt), ref, S, fmt, B.chain_fwd(d))
    assert _rejected(_rounded(got, fmt), ref, S, fmt, B.chain_fwd(d))


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_lost_last_wgrad_split_rejected(fmt):
    """The sixteen-split one-tap record: the last split's pixels left out of the sum, with operands drawn through each
    half format (they are exact in both; the weight gradient itself is fp32 in either)."""
    rec = _record(EDGE_WGRAD, "onetap:split")
    d, splits = rec["desc"], rec["splits"]
    assert splits > 1
    dt = {"bf16": torch.bfloat16, "f16": torch.float16}[fmt]
    g = torch.Generator().manual_seed({"bf16": 14, "f16": 15}[fmt])
    x = R.draw((d["N"], d["Cin"], d["Hin"], d["Win"]), g).to(dt).float()
    gy = R.draw((d["N"], d["Cout"], d["Hout"], d["Wout"]), g).to(dt).float()
    ref, S = R.wgrad(d, x, gy)
    Q = d["N"] * d["Hout"] * d["Wout"]
    nhwc = gy.permute(0, 2, 3, 1).contiguous()
    nhwc.view(Q, d["Cout"])[Q - Q // splits:] = 0
    got, _ = R.wgrad(d, x, nhwc.permute(0, 3, 1, 2))
    assert not _rejected(ref.float().double(), ref, S, "f32", B.chain_wgrad(d))
    assert _rejected(got.float().double(), ref, S, "f32", B.chain_wgrad(d))
