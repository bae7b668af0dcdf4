"""The fp64 comparator of tests/test_window_kernels_gpu.py must catch the bugs it is there for (no GPU).

At real geometries of tests/window_geometries.json, fp64 "faulty outputs" are built from the reference -- the kinds of
mistake an MFMA convolution makes at borders, ragged tiles, sub-pixel classes, split-K partials, statistics rows and
split weight gradients -- and oracle/bounds.py must reject each one, while the unfaulted reference rounded to the
output format passes.
"""
import numpy as np
import pytest
import torch

from oracle import bounds as B
from oracle import conv_ref as R
from oracle import window as WG

CONV = WG.conv_entries()


def _pick(entry, kernel=None, **fields):
    for r in CONV:
        if r["entry"] == entry and (kernel is None or r["kernel"] == kernel) and \
                all(r["desc"][k] == v for k, v in fields.items()):
            return r
    raise LookupError((entry, kernel, fields))


def _operands(d, seed):
    g = torch.Generator().manual_seed(seed)
    x = R.draw((d["N"], d["Cin"], d["Hin"], d["Win"]), g)
    w = R.draw(R.weight_shape(d), g, R.weight_scale(d))
    return x, w


def _rounded(ref, fmt):
    dt = {"bf16": torch.bfloat16, "f16": torch.float16}[fmt]
    return ref.to(dt).double()


def _rejected(got, ref, S, fmt, chain):
    ok, ratio, _, _ = B.check(got.numpy(), ref.numpy(), S.numpy(), fmt, chain)
    return not ok


@pytest.fixture(scope="module")
def k9216():
    """The 1024 -> 1024 reflection-padded 3x3 at 32 x 64 (K = 9216, split-K workspace): fp64 reference."""
    rec = _pick("fwd_ws", "conv3x3_patch_kernel", Cin=1024, Cout=1024, pad_mode=1)
    d = rec["desc"]
    x, w = _operands(d, 1)
    ref, S = R.forward(d, x, w)
    xp, weff, _, _ = R.effective(d, x, w)
    return d, xp, weff, ref, S


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_unfaulted_rounded_reference_passes(k9216, fmt):
    d, _, _, ref, S = k9216
    assert not _rejected(_rounded(ref, fmt), ref, S, fmt, B.chain_fwd(d))


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("where", ["row", "col"])
def test_missing_tap_chunk_on_border_rejected(k9216, fmt, where):
    """Tap (ky, kx) = (0, 1) of input channels 0..63 left out along output row 0 / column 0."""
    d, xp, weff, ref, S = k9216
    ky, kx = 0, 1
    wt = weff[:, :64, ky, kx].double()                        # [Cout, 64]
    got = ref.clone()
    if where == "row":
        xs = xp[0, :64, ky, kx:kx + d["Wout"]].double()       # [64, Wout]
        got[0, 0] -= (wt @ xs).T
    else:
        xs = xp[0, :64, ky:ky + d["Hout"], kx].double()       # [64, Hout]
        got[0, :, 0] -= (wt @ xs).T
    assert _rejected(_rounded(got, fmt), ref, S, fmt, B.chain_fwd(d))


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_lost_split_k_partial_rejected(k9216, fmt):
    """One 128-channel output tile (first 128 pixels) keeps only the first half of its K range."""
    d, xp, weff, ref, S = k9216
    half = dict(d, Cin=d["Cin"] // 2)
    part, _ = R.forward(dict(half, pad_mode=0, pad_h=0, pad_w=0, Hin=xp.shape[2], Win=xp.shape[3]),
                        xp[:, :half["Cin"]], weff[:, :half["Cin"]])
    got = ref.clone()
    flat, pflat = got.view(-1, d["Cout"]), part.view(-1, d["Cout"])
    flat[:128, :128] = pflat[:128, :128]
    assert _rejected(_rounded(got, fmt), ref, S, fmt, B.chain_fwd(d))


@pytest.fixture(scope="module")
def ragged():
    """64 -> 128 4x4 / stride 2 on the 257 x 513 gradient map, 3 samples, statistics per sample (ragged tiles)."""
    rec = _pick("fwd_ws", "conv_igemm_kernel", Cin=64, Hin=257, Win=513, Cout=128, N=3, stats_per_sample=1)
    d = rec["desc"]
    x, w = _operands(d, 2)
    ref, S = R.forward(d, x, w)
    return d, ref, S


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_ragged_last_tile_shift_rejected(ragged, fmt):
    """The last (ragged) 128-pixel tile of the batch written one pixel late."""
    d, ref, S = ragged
    P = d["N"] * d["Hout"] * d["Wout"]
    start = (P - 1) // 128 * 128
    assert start < P - 1
    got = ref.clone()
    flat = got.view(-1, d["Cout"])
    flat[start + 1:] = ref.view(-1, d["Cout"])[start:P - 1]
    assert not _rejected(_rounded(ref, fmt), ref, S, fmt, B.chain_fwd(d))
    assert _rejected(_rounded(got, fmt), ref, S, fmt, B.chain_fwd(d))


def _stats_rows(d, ref, S, tp=128):
    """Reference statistics rows (per-sample tiles of tp pixels) and the summed bound terms."""
    hw = d["Hout"] * d["Wout"]
    per = -(-hw // tp)
    r2, s2 = ref.reshape(-1, d["Cout"]).numpy(), S.reshape(-1, d["Cout"]).numpy()
    terms = B.stats_terms(r2, s2, B.chain_fwd(d))
    rows = [(s * hw + t * tp, s * hw + min(hw, (t + 1) * tp)) for s in range(d["N"]) for t in range(per)]
    acc = [np.stack([q[a:b].sum(0) for a, b in rows]) for q in terms]
    return acc


def test_statistics_missing_last_row_rejected(ragged):
    d, ref, S = ragged
    acc = _stats_rows(d, ref, S)
    exact = np.stack([acc[0], acc[1]], 1).astype(np.float32).astype(np.float64)   # fp32 rows of the exact sums
    assert B.check_stats(exact, acc)[0]
    faulty = exact.copy()
    faulty[-1] = 0
    assert not B.check_stats(faulty, acc)[0]


@pytest.fixture(scope="module")
def wgrad3():
    """Weight gradient of the 64 -> 128 4x4 / stride 2 convolution at 257 x 513, 3 samples (99459 pixels)."""
    rec = _pick("wgrad", Cin=64, Hin=257, Win=513, Cout=128, N=3)
    d = rec["desc"]
    g = torch.Generator().manual_seed(3)
    x = R.draw((d["N"], d["Cin"], d["Hin"], d["Win"]), g)
    gy = R.draw((d["N"], d["Cout"], d["Hout"], d["Wout"]), g)
    ref, S = R.wgrad(d, x, gy)
    return d, x, gy, ref, S


def test_wgrad_unfaulted_passes(wgrad3):
    d, _, _, ref, S = wgrad3
    assert not _rejected(ref.float().double(), ref, S, "f32", B.chain_wgrad(d))


@pytest.mark.parametrize("lost", ["last_split", "last_ragged_row"])
def test_wgrad_missing_segment_rejected(wgrad3, lost):
    """The last of MAX_SPLIT pixel splits, or the last output row of the last sample, left out of the sum."""
    d, x, gy, ref, S = wgrad3
    g = gy.clone()
    if lost == "last_split":
        P = d["N"] * d["Hout"] * d["Wout"]
        seg = -(-P // B.MAX_SPLIT)
        nhwc = g.permute(0, 2, 3, 1).contiguous()
        nhwc.view(P, d["Cout"])[P - seg:] = 0                  # (pixels in NHWC order)
        g = nhwc.permute(0, 3, 1, 2)
    else:
        g[-1, :, -1] = 0
    got, _ = R.wgrad(d, x, g)
    assert _rejected(got.float().double(), ref, S, "f32", B.chain_wgrad(d))


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_subpixel_class_with_neighbour_taps_rejected(fmt):
    """A 4x4 / stride-2 transposed convolution whose odd-column class used the even class's taps."""
    rec = _pick("fwd_ws", "conv_igemm_classes_kernel", Cin=256, Hin=33, Win=65, Cout=128, kh=4, kw=4, transposed=1)
    d = rec["desc"]
    x, w = _operands(d, 4)
    ref, S = R.forward(d, x, w)
    wrong, _ = R.forward(d, x, w[..., [1, 0, 3, 2]])
    got = ref.clone()
    got[:, :, 1::2] = wrong[:, :, 1::2]
    assert not _rejected(_rounded(ref, fmt), ref, S, fmt, B.chain_fwd(d))
    assert _rejected(_rounded(got, fmt), ref, S, fmt, B.chain_fwd(d))


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_bn_dgamma_accumulated_twice_rejected(fmt):
    """BatchNorm backward of a later sample group (params= accumulation, LeakyReLU 0.2) at the window's 2145-pixel,
    256-channel discriminator geometry: a dgamma added twice onto the earlier group's is rejected; the fp64 result
    rounded to the kernel's formats passes."""
    from oracle import bn_ref as BR
    rec = next(r for r in WG.bn_entries() if r["entry"] == "ir2rgb_bn_bwd" and r["args"][10:13] == [2145, 256, 34])
    P, C = rec["args"][10], rec["args"][11]
    g = torch.Generator().manual_seed(5)
    y = (R.draw((P, C), g) * 1.5 + 0.3).to(torch.bfloat16).double().numpy()
    gz = R.draw((P, C), g).double().numpy()
    mean = y.mean(0).astype(np.float32).astype(np.float64)
    invstd = (1.0 / np.sqrt(y.var(0) + 1e-5)).astype(np.float32).astype(np.float64)
    gamma = torch.rand(C, generator=g).double().numpy() + 0.5
    scale = (gamma * invstd).astype(np.float32).astype(np.float64)
    shift = (0.1 - mean * scale).astype(np.float32).astype(np.float64)
    gz[~BR.sign_safe(y, scale, shift)] = 0
    base = (torch.randn(C, generator=g).double().numpy(), torch.randn(C, generator=g).double().numpy())
    ref = BR.bwd(gz, y, scale, shift, mean, invstd, 2, fmt, base)
    dt = {"bf16": torch.bfloat16, "f16": torch.float16}[fmt]
    assert not BR.rejects(torch.from_numpy(ref["gy"][0]).to(dt).double().numpy(), ref["gy"])
    for name in ("dgamma", "dbeta"):
        assert not BR.rejects(ref[name][0].astype(np.float32), ref[name])
    twice = ref["dgamma"][0] + (ref["dgamma"][0] - base[0])
    assert BR.rejects(twice.astype(np.float32), ref["dgamma"])
