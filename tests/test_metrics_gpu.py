"""ir2rgb_video_metrics_u8 (csrc/video_metrics.hip) on the GPU against ``ir2rgb_amd.metrics.ssim_reference`` computed on the
CPU, within the bounds ``metrics.py`` derives from the formula (ssim_bound, l2_bound, RANGE_BOUND): every shape at which the
kernels take another path (one window, one tile, a pixel more and less than a tile, several tiles, the full 512x1024 frame,
frames whose byte size is and is not a multiple of 4), the four kinds of input of tests/test_metrics_cpu.py, batches,
given ranges, streams, workspace reuse, and ``VideoTranslator.evaluate`` end to end."""
import pytest
import torch

from test_metrics_cpu import FULL, KINDS, assert_rows_close, make_pair, reference, small_shapes

pytestmark = pytest.mark.gpu


def _score(dev, orig, pred, data_range="reference"):
    from ir2rgb_amd import metrics
    return metrics.video_metrics(orig.to(dev), pred.to(dev), data_range).cpu()


@pytest.mark.parametrize("kind", KINDS)
def test_small_shapes_match_the_reference(dev, kind):
    for i, (H, W) in enumerate(small_shapes()):
        orig, pred, want = reference(kind, H, W, 100 + i)
        got = _score(dev, orig, pred)
        assert got.shape == (1, 3) and got.dtype == torch.float64
        assert_rows_close(got[0], want, H, W, f"{kind} gpu")
        if kind == "identical":
            assert float(got[0, 1]) == 0.0


@pytest.mark.parametrize("kind", ("random", "smooth"))
def test_full_frame_matches_the_reference(dev, kind):
    H, W = FULL
    orig, pred, want = reference(kind, H, W, 100 + len(small_shapes()))
    assert_rows_close(_score(dev, orig, pred)[0], want, H, W, f"{kind} gpu")


def test_all_black_pair_is_nan(dev):
    black = torch.zeros(9, 13, 3, dtype=torch.uint8)
    row = _score(dev, black, black)[0]
    assert torch.isnan(row[0]) and float(row[1]) == 0.0 and float(row[2]) == 0.0


def _batch():
    pairs = [make_pair(k, 40, 52, 7 + i) for i, k in enumerate(("random", "smooth", "flat"))]
    return torch.stack([p[0] for p in pairs]), torch.stack([p[1] for p in pairs])


def test_batch_rows_are_per_frame_and_permute_bit_exactly(dev):
    from ir2rgb_amd import metrics
    O, P = _batch()
    want = metrics.ssim_reference(O, P)
    got = _score(dev, O, P)
    for n in range(3):
        assert_rows_close(got[n], want[n], 40, 52, f"batch row {n}")
    perm = [2, 0, 1]
    assert torch.equal(_score(dev, O[perm].contiguous(), P[perm].contiguous()), got[perm])
    for n in range(3):
        assert torch.equal(_score(dev, O[n], P[n])[0], got[n])           # frames never mix


def test_given_ranges(dev):
    from ir2rgb_amd import metrics
    O, P = _batch()
    rng = torch.tensor([0.75, 1.0, 2.0], dtype=torch.float64)
    for given, want in ((1.0, metrics.ssim_reference(O, P, 1.0)), (rng, metrics.ssim_reference(O, P, rng)),
                        (rng.to(dev), metrics.ssim_reference(O, P, rng))):
        got = _score(dev, O, P, given)
        assert torch.equal(got[:, 2], want[:, 2])                           # a given range is handed through untouched
        for n in range(3):
            assert_rows_close(got[n], want[n], 40, 52, "given range")
    assert not torch.equal(_score(dev, O, P, 1.0)[:, 0], _score(dev, O, P)[:, 0])


def test_repeatable_on_any_stream_with_a_reused_workspace(dev):
    from ir2rgb_amd import _lib, metrics
    big = [t.to(dev) for t in make_pair("random", 64, 128, 11)]
    tiny = [t.to(dev) for t in make_pair("smooth", 7, 7, 12)]
    first = metrics.video_metrics(*big)
    assert torch.equal(metrics.video_metrics(*big), first)                  # two calls, the same bits
    tiny_first = metrics.video_metrics(*tiny)
    assert torch.equal(metrics.video_metrics(*big), first)                  # large, 7x7, large again: nothing stale
    assert torch.equal(metrics.video_metrics(*tiny), tiny_first)
    assert_rows_close(tiny_first[0].cpu(), metrics.ssim_reference(tiny[0].cpu(), tiny[1].cpu())[0], 7, 7, "tiny")
    # one caller-owned workspace through the C ABI, larger than needed and full of NaN, shared by both shapes
    lib = _lib.lib()
    ws = torch.full((lib.ir2rgb_video_metrics_workspace_bytes(1, 64, 128) // 8 + 5,), float("nan"), dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    for pair, want in ((big, first), (tiny, tiny_first), (big, first)):
        out = torch.empty(1, 3, dtype=torch.float64, device=dev)
        H, W = pair[0].shape[:2]
        assert lib.ir2rgb_video_metrics_u8(pair[0], pair[1], None, out, ws, ws.numel() * 8, 1, H, W, stream) == 0
        assert torch.equal(out, want)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        other = metrics.video_metrics(*big)
    side.synchronize()
    assert torch.equal(other, first)


@pytest.mark.parametrize("H,W", [(9, 13), (8, 16)])
def test_both_scores_alternate_on_one_workspace_cache(dev, H, W):
    """``video_metrics`` and ``warp_error`` share one workspace cache.  Called in turn at the same N, H, W on the same
    stream, and once more on a second stream, each repeats its first result bit for bit and stays within the bounds of its
    CPU reference.  On the first stream ``warp_error`` goes first: a cache keyed without the entry would then hand the
    SSIM call the smaller warp-error buffer, which the library refuses.  The cache holds, per stream, two distinct buffers
    of the sizes the two entries ask for.  9x13 has an odd byte count (the scalar form of both reduce kernels), 8x16 takes
    the 4-pixel form."""
    import test_warp_error_cpu as warp
    from ir2rgb_amd import _lib, metrics
    frames = [make_pair(k, H, W, 31 + i) for i, k in enumerate(("random", "smooth"))]
    O, P = torch.stack([f[0] for f in frames]), torch.stack([f[1] for f in frames])
    pairs = [warp.reference("random", "fractional", H, W), warp.reference("consistent", "binary", H, W)]
    prev, cur, flow, weight = (torch.stack([p[j] for p in pairs]) for j in range(4))
    ssim_want = metrics.ssim_reference(O, P)
    ssim_in, warp_in = [O.to(dev), P.to(dev)], [t.to(dev) for t in (prev, cur, flow, weight)]

    def check(ssim_got, warp_got, what):
        for n in range(2):
            assert_rows_close(ssim_got[n].cpu(), ssim_want[n], H, W, f"{what} ssim row {n}")
            warp.assert_rows_close(warp_got[n].cpu(), pairs[n][4], pairs[n][5], f"{what} warp row {n}")

    def cached(stream):
        """The two buffers the cache holds for (stream, 2, H, W): each of the size its own entry asks for."""
        lib, ws = _lib.lib(), {}
        for entry in ("video_metrics", "warp_error"):
            ws[entry] = metrics._WORKSPACES[(entry, dev.index, stream, 2, H, W)]
            assert ws[entry].numel() * 8 == getattr(lib, f"ir2rgb_{entry}_workspace_bytes")(2, H, W)
        assert ws["video_metrics"].numel() > ws["warp_error"].numel()
        assert ws["video_metrics"].data_ptr() != ws["warp_error"].data_ptr()
        return ws

    # this stream: warp_error first, so that the SSIM call finds the smaller buffer already cached for (stream, N, H, W)
    warp_first, ssim_first = metrics.warp_error(*warp_in), metrics.video_metrics(*ssim_in)
    check(ssim_first, warp_first, "first")
    assert torch.equal(metrics.warp_error(*warp_in), warp_first) and torch.equal(metrics.video_metrics(*ssim_in), ssim_first)
    main = cached(_lib.current_stream(ssim_first))
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):               # a second stream, the other order
        again = [(metrics.video_metrics(*ssim_in), metrics.warp_error(*warp_in)) for _ in range(2)]
        side_key = _lib.current_stream(ssim_first)
    side.synchronize()
    for s, w in again:
        assert torch.equal(s, ssim_first) and torch.equal(w, warp_first)
    check(*again[0], "side stream")
    other = cached(side_key)
    assert all(main[e].data_ptr() != other[e].data_ptr() for e in main)        # streams never share a buffer


def test_frames_far_into_a_long_batch(dev):
    """Byte offsets of the last frames lie past 2^31: they score what the same frames score alone."""
    from ir2rgb_amd import metrics
    N, H, W = 700, 1024, 1024
    assert (N - 1) * H * W * 3 > 2 ** 31
    g = torch.Generator(device=dev).manual_seed(3)
    O = torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8, device=dev)
    P = torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8, device=dev)
    rows = metrics.video_metrics(O, P)
    for n in (0, N - 1):
        assert torch.equal(rows[n], metrics.video_metrics(O[n], P[n])[0])
    assert bool(torch.isfinite(rows).all()) and not torch.equal(rows[N - 1], rows[N - 2])


def test_evaluate_is_translate_plus_videoscore(dev):
    from ir2rgb_amd import metrics, networks as N
    from ir2rgb_amd.inference import VideoTranslator
    tG, H, W = 3, 32, 64
    torch.manual_seed(21)
    netG = [N.build_generator_module(3 * tG, 3, 3 * (tG - 1), 16, "composite", 3, "batch", 0, gen_blocks=9, n_blocks_local=3,
                                     fg=False, no_flow=False, n_local_enhancers=1, feat_num=3)]
    g = torch.Generator().manual_seed(22)
    frames = list(torch.randint(0, 256, (6, H, W, 3), generator=g, dtype=torch.uint8))
    targets = list(torch.randint(0, 256, (6, H, W, 3), generator=g, dtype=torch.uint8))
    tr = VideoTranslator(dev, H, W, netG=netG, n_scales_spatial=1, ngf=16)
    plain = [o.clone() for o in tr.translate(frames)]
    assert len(plain) == 6 - (tG - 1)
    score = tr.evaluate(frames, targets)
    assert isinstance(score, metrics.VideoScore) and score.frames == len(plain)
    by_hand = metrics.VideoScore()
    outs = []
    for k, out in enumerate(tr.translate(frames)):
        outs.append(out)
        by_hand.add(targets[tG - 1 + k].to(dev), out)
    for a, b in zip(plain, outs):
        assert torch.equal(a, b)                                            # translate() is unchanged by having been scored
    res, want = score.result(), by_hand.result()
    assert torch.equal(res["per_frame"], want["per_frame"]) and res["per_frame"].shape == (len(plain), 3)
    assert res["ssim"] == want["ssim"] and res["l2"] == want["l2"] and res["frames"] == len(plain)
    ref = torch.stack([metrics.ssim_reference(targets[tG - 1 + k], o.cpu())[0] for k, o in enumerate(outs)])
    for k in range(len(outs)):
        assert_rows_close(res["per_frame"][k].cpu(), ref[k], H, W, f"evaluate frame {k}")
    with pytest.raises(ValueError, match="targets"):
        tr.evaluate(frames, targets[:4])
