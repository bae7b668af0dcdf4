"""ir2rgb_colour_metrics_u8 (csrc/colour_metrics.hip) on the GPU against ``ir2rgb_amd.metrics.colour_reference`` computed
on the CPU, within the bound ``metrics.colour_bound`` derives from the formula and with ``mse`` bit for bit: every shape and
image kind of tests/test_colour_metrics_cpu.py (the dword and the one-pixel form, one and several workgroups per frame, the
full 512x1024 frame and its grid-stride loop, misaligned bases), batches, streams, identical frames, and
``VideoTranslator.evaluate(colour=True)`` end to end."""
import math

import pytest
import torch

from test_colour_metrics_cpu import COLUMNS, FULL, KINDS, SHAPES, assert_rows_close, batch, make_pair, reference

pytestmark = pytest.mark.gpu


def _score(dev, orig, pred):
    from ir2rgb_amd import metrics
    return metrics.colour_metrics(orig.to(dev), pred.to(dev)).cpu()


@pytest.mark.parametrize("kind", KINDS)
def test_small_shapes_match_the_reference(dev, kind):
    for H, W in SHAPES:
        orig, pred, want, bound = reference(kind, H, W)
        got = _score(dev, orig, pred)
        assert got.shape == (1, 5) and got.dtype == torch.float64
        assert_rows_close(got[0], want, bound, f"{kind} {(H, W)} gpu")


def test_full_frame_matches_the_reference(dev):
    H, W = FULL
    orig, pred, want, bound = reference("random", H, W)
    assert_rows_close(_score(dev, orig, pred)[0], want, bound, "random full frame gpu")


def test_misaligned_bases_take_the_one_pixel_form(dev):
    """A W % 4 == 0 frame that starts one byte into a larger buffer: no dword load may be issued on it.  Another order of
    the per-thread sums, so the aligned call's row within the bound, the reference's too, and mse bit for bit."""
    from ir2rgb_amd import metrics
    H, W = 16, 32
    orig, pred, want, bound = reference("random", H, W)

    def shifted(t):
        buf = torch.zeros(t.numel() + 1, dtype=t.dtype, device=dev)
        buf[1:] = t.to(dev).flatten()
        v = buf[1:].view(t.shape)
        assert v.is_contiguous() and v.data_ptr() % 4 != 0
        return v

    aligned = _score(dev, orig, pred)[0]
    for o, p, what in ((shifted(orig), shifted(pred), "both off a dword"), (orig.to(dev), shifted(pred), "pred off a dword"),
                       (shifted(orig), pred.to(dev), "orig off a dword")):
        got = metrics.colour_metrics(o, p).cpu()[0]
        assert_rows_close(got, want, bound, what + " vs reference")
        assert_rows_close(got, aligned, bound, what + " vs aligned")


def test_batch_rows_are_per_frame_and_permute_bit_exactly(dev):
    from ir2rgb_amd import metrics
    O, P = batch(32, 36)
    want = metrics.colour_reference(O, P)
    got = _score(dev, O, P)
    for n in range(3):
        assert_rows_close(got[n], want[n], metrics.colour_bound(32, 36, want[n, 1]), f"batch row {n}")
    perm = [2, 0, 1]
    assert torch.equal(_score(dev, O[perm].contiguous(), P[perm].contiguous()), got[perm])
    for n in range(3):
        assert torch.equal(_score(dev, O[n], P[n])[0], got[n])                      # frames never mix


def test_frames_of_a_long_ragged_batch(dev):
    """300 frames of 7x13 (273 bytes each: no frame but every fourth starts on a dword): each scores what it scores alone."""
    N, H, W = 300, 7, 13
    g = torch.Generator().manual_seed(9)
    O = torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8)
    P = torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8)
    rows = _score(dev, O, P)
    assert rows.shape == (N, 5) and bool(torch.isfinite(rows).all())
    for n in (0, 1, 2, 3, 150, 298, 299):
        assert torch.equal(_score(dev, O[n], P[n])[0], rows[n]), n
    assert not torch.equal(rows[298], rows[299])


def test_repeatable_on_any_stream(dev):
    from ir2rgb_amd import metrics
    big = [t.to(dev) for t in reference("random", 64, 128)[:2]]
    tiny = [t.to(dev) for t in reference("grey", 1, 5)[:2]]
    first, tiny_first = metrics.colour_metrics(*big), metrics.colour_metrics(*tiny)
    assert torch.equal(metrics.colour_metrics(*big), first) and torch.equal(metrics.colour_metrics(*tiny), tiny_first)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        other, tiny_other = metrics.colour_metrics(*big), metrics.colour_metrics(*tiny)
    side.synchronize()
    assert torch.equal(other, first) and torch.equal(tiny_other, tiny_first)


def test_identical_frames_score_zero_and_infinite_psnr(dev):
    for kind, (H, W) in (("random", (7, 13)), ("dark", (16, 32)), ("grey", (1, 1)), ("random", (64, 128))):
        orig = reference(kind, H, W)[0]
        row = _score(dev, orig, orig.clone())[0].tolist()
        assert row == [0.0, math.inf, 0.0, 0.0, 0.0], (kind, H, W, row)
    O, P = batch()
    P = P.clone()
    P[1] = O[1]                                                 # one identical pair inside a batch: its row only
    rows, clean = _score(dev, O, P), _score(dev, *batch())
    assert rows[1].tolist() == [0.0, math.inf, 0.0, 0.0, 0.0] and torch.equal(rows[0], clean[0]) and torch.equal(rows[2], clean[2])


def test_srgb_table_on_the_device_is_the_hosts(dev):
    from ir2rgb_amd import metrics
    t = metrics.srgb_table(dev)
    assert t.device == dev and t.dtype == torch.float64 and metrics.srgb_table(dev) is t
    assert torch.equal(t.cpu(), metrics.srgb_table())


def _toy_translator(dev, H, W, tG=3):
    from ir2rgb_amd import networks as N
    from ir2rgb_amd.inference import VideoTranslator
    torch.manual_seed(21)
    netG = [N.build_generator_module(3 * tG, 3, 3 * (tG - 1), 16, "composite", 3, "batch", 0, gen_blocks=9, n_blocks_local=3,
                                     fg=False, no_flow=False, n_local_enhancers=1, feat_num=3)]
    return VideoTranslator(dev, H, W, netG=netG, n_scales_spatial=1, ngf=16)


def test_evaluate_in_colour(dev):
    from ir2rgb_amd import metrics
    tG, H, W = 3, 32, 64
    g = torch.Generator().manual_seed(22)
    frames = list(torch.randint(0, 256, (6, H, W, 3), generator=g, dtype=torch.uint8))
    targets = list(torch.randint(0, 256, (6, H, W, 3), generator=g, dtype=torch.uint8))
    tr = _toy_translator(dev, H, W, tG)
    plain = [o.clone() for o in tr.translate(frames)]
    without = tr.evaluate(frames, targets).result()
    assert list(without) == ["ssim", "l2", "frames", "per_frame"]
    res = tr.evaluate(frames, targets, colour=True).result()
    assert list(res) == ["ssim", "l2", "frames", "per_frame", "mse", "psnr", "delta_e", "delta_l", "delta_c", "per_frame_colour"]
    assert torch.equal(res["per_frame"], without["per_frame"]) and res["ssim"] == without["ssim"]
    pc = res["per_frame_colour"]
    assert pc.shape == (len(plain), 5) and pc.dtype == torch.float64 and pc.device == dev
    for k, out in enumerate(plain):
        target = targets[tG - 1 + k]
        assert torch.equal(pc[k], metrics.colour_metrics(target.to(dev), out)[0])
        want = metrics.colour_reference(target, out.cpu())[0]
        assert_rows_close(pc[k].cpu(), want, metrics.colour_bound(H, W, want[1]), f"evaluate frame {k}")
    assert [res[c] for c in COLUMNS] == pc.mean(0).tolist()
