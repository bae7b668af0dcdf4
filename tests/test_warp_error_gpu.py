"""ir2rgb_warp_error_u8 (csrc/warp_error.hip) on the GPU against ``ir2rgb_amd.metrics.warp_error_reference`` computed on
the CPU, within the bound ``metrics.warp_bound`` derives from the formula: every shape, image kind and weight form of
tests/test_warp_error_cpu.py (the 4-pixel and the scalar form, one and several workgroups per pair, the full 512x1024
frame, misaligned bases), batches, non-finite flows, streams, workspace reuse, offsets past 2^31, and
``VideoTranslator.evaluate(temporal=...)`` end to end."""
import pytest
import torch

from test_warp_error_cpu import (FULL, KINDS, SHAPES, WEIGHTS, assert_rows_close, batch, check_nonfinite_rows, huge_flow_rows,
                                 make_flow, make_weight, nonfinite_cases, reference)

pytestmark = pytest.mark.gpu


def _score(dev, prev, cur, flow, weight):
    from ir2rgb_amd import metrics
    return metrics.warp_error(prev.to(dev), cur.to(dev), flow.to(dev), weight.to(dev) if weight is not None else None).cpu()


@pytest.mark.parametrize("wkind", WEIGHTS)
@pytest.mark.parametrize("kind", KINDS)
def test_small_shapes_match_the_reference(dev, kind, wkind):
    for H, W in SHAPES:
        prev, cur, flow, weight, want, bound = reference(kind, wkind, H, W)
        got = _score(dev, prev, cur, flow, weight)
        assert got.shape == (1, 3) and got.dtype == torch.float64
        assert_rows_close(got[0], want, bound, f"{kind} {wkind} {(H, W)} gpu")
        if wkind == "none":
            assert float(got[0, 2]) == 1.0


def test_full_frame_matches_the_reference(dev):
    H, W = FULL
    prev, cur, flow, weight, want, bound = reference("random", "binary", H, W)
    assert_rows_close(_score(dev, prev, cur, flow, weight)[0], want, bound, "random binary full frame gpu")


def test_misaligned_bases_take_the_scalar_form(dev):
    """A W % 4 == 0 frame whose flow, weight and frames start one element into a larger buffer: no 16-byte or dword load
    may be issued on them, and the result is the reference's."""
    from ir2rgb_amd import metrics
    H, W = 16, 32
    prev, cur, flow, weight, want, bound = reference("random", "fractional", H, W)

    def shifted(t):
        buf = torch.zeros(t.numel() + 1, dtype=t.dtype, device=dev)
        buf[1:] = t.to(dev).flatten()
        v = buf[1:].view(t.shape)
        assert v.is_contiguous() and v.data_ptr() % (16 if t.dtype == torch.float32 else 4) != 0
        return v

    got = metrics.warp_error(shifted(prev), shifted(cur), shifted(flow), shifted(weight)).cpu()
    assert_rows_close(got[0], want, bound, "misaligned bases")
    got = metrics.warp_error(prev.to(dev), shifted(cur), flow.to(dev), None).cpu()     # the frame alone is off a dword
    ref = reference("random", "none", H, W)
    assert_rows_close(got[0], ref[4], ref[5], "misaligned cur")


def test_batch_rows_are_per_pair_and_permute_bit_exactly(dev):
    from ir2rgb_amd import metrics
    P, C, Fl, Wt = batch(40, 52)
    want, bound = metrics.warp_error_reference(P, C, Fl, Wt), metrics.warp_bound(40, 52, Fl, Wt)
    got = _score(dev, P, C, Fl, Wt)
    for n in range(3):
        assert_rows_close(got[n], want[n], bound[n], f"batch row {n}")
    perm = [2, 0, 1]
    assert torch.equal(_score(dev, *(t[perm].contiguous() for t in (P, C, Fl, Wt))), got[perm])
    for n in range(3):
        assert torch.equal(_score(dev, P[n], C[n], Fl[n], Wt[n])[0], got[n])            # pairs never mix


def test_nonfinite_flow_and_weight_stay_in_their_pair(dev):
    P, C, Fl, Wt = batch()
    clean = _score(dev, P, C, Fl, Wt)
    huge = huge_flow_rows(lambda *a: _score(dev, *a))
    for name, (f, w) in nonfinite_cases().items():
        check_nonfinite_rows(name, _score(dev, P, C, f, w), clean, huge)
    zero = _score(dev, P, C, Fl, torch.zeros_like(Wt))
    assert bool((zero[:, 0] == 0).all()) and bool(torch.isnan(zero[:, 1]).all()) and bool((zero[:, 2] == 0).all())


def test_repeatable_on_any_stream_with_a_shared_workspace(dev):
    from ir2rgb_amd import _lib, metrics
    big = [t.to(dev) for t in reference("random", "fractional", 64, 128)[:4]]
    tiny = [t.to(dev) for t in reference("consistent", "binary", 2, 3)[:4]]
    first = metrics.warp_error(*big)
    assert torch.equal(metrics.warp_error(*big), first)                     # two calls, the same bits
    tiny_first = metrics.warp_error(*tiny)
    assert torch.equal(metrics.warp_error(*big), first) and torch.equal(metrics.warp_error(*tiny), tiny_first)
    # one caller-owned workspace through the C ABI, larger than needed and full of NaN, shared by both shapes, on a side stream
    lib = _lib.lib()
    ws = torch.full((lib.ir2rgb_warp_error_workspace_bytes(1, 64, 128) // 8 + 5,), float("nan"), dtype=torch.float64, device=dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for pair, want in ((big, first), (tiny, tiny_first), (big, first)):
            out = torch.empty(1, 3, dtype=torch.float64, device=dev)
            H, W = pair[0].shape[:2]
            assert lib.ir2rgb_warp_error_u8(pair[0], pair[1], pair[2], pair[3], out, ws, ws.numel() * 8, 1, H, W, side.cuda_stream) == 0
            side.synchronize()
            assert torch.equal(out, want)
        other = metrics.warp_error(*big)
    side.synchronize()
    assert torch.equal(other, first)


def test_pairs_far_into_a_long_batch(dev):
    """Element (= byte) offsets of the last frames and byte offsets of the last flows lie past 2^31: they score what the
    same pairs score alone."""
    from ir2rgb_amd import metrics
    N, H, W = 700, 1024, 1024
    assert (N - 1) * H * W * 3 > 2 ** 31 and (N - 1) * H * W * 2 * 4 > 2 ** 31
    g = torch.Generator(device=dev).manual_seed(3)
    P = torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8, device=dev)
    C = torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8, device=dev)
    Fl = torch.randn((N, 2, H, W), generator=g, dtype=torch.float32, device=dev) * 3
    rows = metrics.warp_error(P, C, Fl)
    for n in (0, N - 1):
        assert torch.equal(rows[n], metrics.warp_error(P[n], C[n], Fl[n])[0])
    assert bool(torch.isfinite(rows).all()) and bool((rows[:, 2] == 1).all()) and not torch.equal(rows[N - 1], rows[N - 2])


def _toy_translator(dev, H, W, tG=3):
    from ir2rgb_amd import networks as N
    from ir2rgb_amd.inference import VideoTranslator
    torch.manual_seed(21)
    netG = [N.build_generator_module(3 * tG, 3, 3 * (tG - 1), 16, "composite", 3, "batch", 0, gen_blocks=9, n_blocks_local=3,
                                     fg=False, no_flow=False, n_local_enhancers=1, feat_num=3)]
    return VideoTranslator(dev, H, W, netG=netG, n_scales_spatial=1, ngf=16)


def test_evaluate_with_a_stub_flow(dev):
    from ir2rgb_amd import metrics
    from ir2rgb_amd.inference import normalise_u8
    tG, H, W = 3, 32, 64
    g = torch.Generator().manual_seed(22)
    frames = list(torch.randint(0, 256, (6, H, W, 3), generator=g, dtype=torch.uint8))
    targets = list(torch.randint(0, 256, (6, H, W, 3), generator=g, dtype=torch.uint8))
    tr = _toy_translator(dev, H, W, tG)
    plain = [o.clone() for o in tr.translate(frames)]
    without = tr.evaluate(frames, targets).result()
    assert list(without) == ["ssim", "l2", "frames", "per_frame"]
    calls = []

    def stub(cur, prev):
        calls.append((cur.clone(), prev.clone()))
        k = len(calls)
        return make_flow(H, W, k).unsqueeze(0).to(dev), make_weight("fractional", H, W, k).unsqueeze(0).to(dev)

    res = tr.evaluate(frames, targets, temporal=stub).result()
    again = [o.clone() for o in tr.translate(frames)]
    for a, b in zip(plain, again):
        assert torch.equal(a, b)                                            # translate() is unchanged by having been scored
    assert torch.equal(res["per_frame"], without["per_frame"]) and res["ssim"] == without["ssim"] and res["l2"] == without["l2"]
    n = len(plain)
    assert res["pairs"] == n - 1 == len(calls) and res["per_pair"].shape == (n - 1, 5) and res["per_pair"].dtype == torch.float64
    for k in range(1, n):
        t_prev, t_cur = targets[tG - 2 + k].to(dev), targets[tG - 1 + k].to(dev)
        assert torch.equal(calls[k - 1][0][0], normalise_u8(t_cur)) and torch.equal(calls[k - 1][1][0], normalise_u8(t_prev))
        flow, conf = make_flow(H, W, k).to(dev), make_weight("fractional", H, W, k).to(dev)
        pred = metrics.warp_error(plain[k - 1], plain[k], flow, conf)[0]
        truth = metrics.warp_error(t_prev, t_cur, flow, conf)[0]
        assert torch.equal(res["per_pair"][k - 1], torch.stack([pred[0], pred[1], truth[0], truth[1], pred[2]]))
        want = metrics.warp_error_reference(plain[k - 1].cpu(), plain[k].cpu(), flow.cpu(), conf.cpu())
        assert_rows_close(pred.cpu(), want[0], metrics.warp_bound(H, W, flow.cpu(), conf.cpu())[0], f"evaluate pair {k}")
    assert [res[c] for c in ("warp_l1", "warp_mse", "truth_warp_l1", "truth_warp_mse", "coverage")] == res["per_pair"].mean(0).tolist()


def test_evaluate_with_a_flownet(dev):
    """The plumbing with the real flow network (seeded; its biases scaled by 0.05 as everywhere in this suite, because the
    reference's random init blows activations up layer by layer): ``conf`` is a 0/1 mask at a size FlowNet2 does not
    resize, and the scores are finite -- warp_mse wherever the mask kept a pixel, NaN (0/0) exactly where it kept none."""
    from ir2rgb_amd.flownet import FlowNet
    tG, H, W = 3, 64, 128
    g = torch.Generator().manual_seed(23)
    frames = list(torch.randint(0, 256, (6, H, W, 3), generator=g, dtype=torch.uint8))
    y, x = torch.arange(H).view(H, 1, 1), torch.arange(W).view(1, W, 1)
    targets = [(128 + 60 * torch.sin(0.11 * (x + k) + 0.07 * y + torch.arange(3).view(1, 1, 3))).round().to(torch.uint8)
               for k in range(6)]
    fn = FlowNet(seed=1, use_graph=False)
    with torch.no_grad():
        for p in fn.flowNet.parameters():
            if p.dim() == 1:
                p.mul_(0.05)
    fn = fn.to(dev)
    seen = []

    def temporal(cur, prev):
        out = fn(cur, prev)
        seen.append(out)
        return out

    tr = _toy_translator(dev, H, W, tG)
    res = tr.evaluate(frames, targets, temporal=temporal).result()
    assert res["pairs"] == 3 == len(seen) and res["per_pair"].shape == (3, 5)
    for flow, conf in seen:
        assert flow.shape == (1, 2, H, W) and conf.shape == (1, 1, H, W) and flow.dtype == conf.dtype == torch.float32
        assert bool(((conf == 0) | (conf == 1)).all()) and bool(torch.isfinite(flow).all())
    pp = res["per_pair"].cpu()
    print("flownet pairs", pp.tolist())
    assert bool(torch.isfinite(pp[:, [0, 2, 4]]).all())
    for k in range(3):
        for c in (1, 3):
            assert bool(torch.isfinite(pp[k, c])) == (float(pp[k, 4]) > 0), (k, c, pp[k].tolist())
