"""Frame scaling on the GPU (ir2rgb_amd.transform.FrameScaler, csrc/frame_scale.hip).  Every step runs in a child process of
its own under its own time limit (``python tests/test_scale_gpu.py <step>``), as in tests/test_inference_gpu.py.  Every
comparison is equality (tolerance 0): the kernels do integer arithmetic on tables computed on the host, and the fp32
epilogue is three correctly rounded operations.  The GPU steps read only tests/golden/scale_cases.npz (outputs recorded
from Pillow) and ``transform.resize_reference``; neither Pillow nor the reference is needed.

  kernels     every golden case, C = 1 and 3, uint8 and normalised fp32 output, canary bands around the destination and the
              workspace: both axes enlarged (dword and scalar rows), reduced (7, 9 and 33 taps and whole-axis windows,
              clipped at both edges), sources narrower than the support, one pass or both skipped, crop (inside, off the edge, larger
              than the image), flip, saturating checkerboards and step edges; three frames in one call against three
              calls; a destination misaligned by one byte
  fullsize    512x640x3 -> 832x1024 and -> 416x512 against resize_reference computed on the CPU in the step
              FrameScaler.from_options for every way the drawn parameters reach the scaler
  translator  camera-size frames through VideoTranslator against frames scaled by resize_reference on the host and pushed
              at the network's size: bit-identical images and histories over 6 frames, use_graph on and off, across a
              reset(), first frame from zeros and from real (camera-size) RGB; evaluate() against video_metrics on
              host-scaled targets; batched calls on the scaler handed in, and on the translator's own, between replays of
              the captured step; the scaling options with a seeded draw
"""
import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
G_OPT = dict(gen_blocks=9, n_blocks_local=3, fg=False, no_flow=False, n_local_enhancers=1, feat_num=3)
TG = 3
GUARD = 32768


def _run(step, seconds):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), step], capture_output=True, text=True, timeout=seconds,
                       cwd=ROOT)
    print(r.stdout[-6000:])
    assert r.returncode == 0, f"step {step} ended with {r.returncode}:\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    assert f"step {step} ok" in r.stdout


def test_scale_kernels_equal_pillow(dev):
    _run("kernels", 300)


def test_full_size_frames_equal_the_restatement(dev):
    _run("fullsize", 300)


def test_translator_takes_camera_size_frames(dev):
    _run("translator", 420)


# =============================================================================================
# the steps (child process)
# =============================================================================================
class Guarded:
    """``n`` elements inside a larger allocation whose neighbourhood holds a canary; ``skew`` shifts the start by that many
    elements (a misaligned base for byte buffers)."""

    def __init__(self, shape, dtype, dev, fill, junk, skew=0):
        n = int(np.prod(shape))
        self.fill = fill
        self.buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev)
        self.t = self.buf[GUARD + skew:GUARD + skew + n].view(shape)
        self.t.fill_(junk)
        self.lo, self.hi = GUARD + skew, GUARD + skew + n

    def intact(self):
        return bool((self.buf[:self.lo] == self.fill).all() and (self.buf[self.hi:] == self.fill).all())


def _normalised(out_u8):
    """[N,H,W,C] uint8 (CPU) -> [N,C,H,W] fp32 by inference.normalise_u8, frame by frame."""
    from ir2rgb_amd.inference import normalise_u8
    return torch.stack([normalise_u8(f) for f in out_u8])


def _scale_checked(sc, src, want_u8, what, skew=0, ws_skew=0):
    """One call per output form with canaries around destination and workspace -> the uint8 result (CPU).  ``skew`` /
    ``ws_skew`` move the uint8 destination / the workspace off the 4-byte boundary by that many bytes."""
    n = src.shape[0]
    hc, wc = sc.out_hw
    assert tuple(want_u8.shape) == (n, hc, wc, sc.channels), what
    need = sc.workspace_bytes(n)
    got_u8 = None
    for normalised in (False, True):
        ws = Guarded((need,), torch.uint8, src.device, 0x5A, 0xC3, skew=ws_skew)
        own = sc._ws.data_ptr()
        if normalised:
            dst = Guarded((n, sc.channels, hc, wc), torch.float32, src.device, 7.0, 3.0)
            want = _normalised(want_u8)
        else:
            dst = Guarded((n, hc, wc, sc.channels), torch.uint8, src.device, 0xA5, 0x3C, skew=skew)
            want = want_u8
        keep = src.clone()
        out = sc(src, out=dst.t, normalised=normalised, workspace=ws.t)
        torch.cuda.synchronize()
        assert out.data_ptr() == dst.t.data_ptr() and sc._ws.data_ptr() == own
        assert torch.equal(out.cpu(), want), f"{what} normalised={normalised}: result differs"
        assert dst.intact(), f"{what} normalised={normalised}: wrote outside the destination"
        assert ws.intact(), f"{what} normalised={normalised}: wrote outside the workspace"
        assert torch.equal(src, keep), what
        if not normalised:
            got_u8 = out.cpu()
    return got_u8


def step_kernels(dev):
    from ir2rgb_amd.transform import FrameScaler
    d = np.load(os.path.join(GOLDEN, "scale_cases.npz"))
    cases = json.loads(str(d["cases"]))
    names = {m["name"] for m in cases}
    assert {"up_dword", "up_scalar", "down_9_7_taps", "down_33_taps", "down_to_1x1", "narrow_source", "from_1x1", "skip_vertical",
            "skip_horizontal", "skip_both", "crop", "crop_off_edge", "crop_larger_than_image", "flip", "flip_crop",
            "checker_down", "checker_up", "steps_down", "steps_up"} <= names
    for m in cases:
        for C in (1, 3):
            src = torch.from_numpy(d[f"{m['name']}/c{C}/src"]).to(dev)
            want = torch.from_numpy(d[f"{m['name']}/c{C}/out"])
            sc = FrameScaler(dev, m["src_hw"], C, m["new_size"], m["crop_size"], m["crop_pos"], m["flip"])
            what = f"{m['name']} C={C} {m['src_hw']} -> {m['new_size'][::-1]}"
            _scale_checked(sc, src, want, what)
            one = sc(src[0])                                            # a single frame, buffers of the scaler's own
            assert torch.equal(one.cpu(), want[0]) and torch.equal(sc(src[0], normalised=True).cpu(), _normalised(want)[0]), what
            if (sc.out_hw[1] * C) % 4 == 0:        # dword rows: a destination or workspace base off by one byte takes the scalar form
                _scale_checked(sc, src, want, what + " misaligned destination", skew=1)
                _scale_checked(sc, src, want, what + " misaligned workspace", ws_skew=1)
        print(f"kernels: {m['name']} exact (C = 1, 3; uint8, fp32)")
    # three frames in one call against three calls (and against Pillow)
    for C in (1, 3):
        parts = [f"{n}/c{C}" for n in ("up_dword", "checker_up", "steps_up")]
        src = torch.from_numpy(np.concatenate([d[p + "/src"] for p in parts])).to(dev)
        want = torch.from_numpy(np.concatenate([d[p + "/out"] for p in parts]))
        sc = FrameScaler(dev, (37, 53), C, (96, 64))
        got = _scale_checked(sc, src, want, f"batch of 3 C={C}")
        for i in range(3):
            assert torch.equal(sc(src[i]).cpu(), got[i]) and torch.equal(sc(src[i:i + 1]).cpu(), got[i:i + 1])
    print("kernels: one call of three frames = three calls")
    _from_options(dev, src)
    with pytest.raises(ValueError):
        sc(src[:, :-1].contiguous())
    with pytest.raises(ValueError):
        sc(src.cpu())
    with pytest.raises(TypeError):
        sc(src.float())


def _from_options(dev, batch):
    """FrameScaler.from_options: img_params' choice carried onto the scaler the way get_transform applies it -- ``resize``
    scales to load_size x load_size whatever new_size says, the crop (position drawn for the rounded new_size) applies only
    in the crop modes, the flip only with is_train and flip -- against transform_reference on the same parameters."""
    import random
    from ir2rgb_amd.transform import FrameScaler, img_params, transform_reference
    src = batch[:2, :, :, :3].contiguous()                                # [2,37,53,3]
    hs, ws = src.shape[1:3]
    seen = set()
    for seed, opt in enumerate((
            dict(dataset_scale="resize", dataset_crop="none", load_size=100, fine_size=64),        # new_size 96x96, scaled to 100x100
            dict(dataset_scale="resize", dataset_crop="crop", load_size=100, fine_size=60, is_train=True, flip=True),
            dict(dataset_scale="scale-height", dataset_crop="scaled-crop", load_size=90, fine_size=40, is_train=True, flip=True),
            dict(dataset_scale="random-scale-width", dataset_crop="crop", load_size=120, fine_size=64, is_train=True, flip=True),
            dict(dataset_scale="random-scale-width", dataset_crop="crop", load_size=120, fine_size=64, is_train=False, flip=True),
            dict(dataset_scale="scale-width", dataset_crop="none", load_size=128, fine_size=64, is_train=True, flip=True),
            dict(dataset_scale="none", dataset_crop="none", is_train=True, flip=True))):
        opt["dataset_mode"] = "ir2rgb"
        rng = (random.Random(40 + seed), np.random.RandomState(40 + seed))
        sc = FrameScaler.from_options(dev, (hs, ws), 3, rng=rng, **opt)
        p = img_params((ws, hs), rng=(random.Random(40 + seed), np.random.RandomState(40 + seed)), **opt)
        assert sc.params == p, opt
        crop = opt["dataset_crop"] != "none"
        flip = bool(p["flip"] and opt.get("is_train") and opt.get("flip"))
        size = (opt["load_size"],) * 2 if opt["dataset_scale"] == "resize" else p["new_size"]
        want = transform_reference(src.cpu(), size, p["crop_size"] if crop else (0, 0), p["crop_pos"] if crop else (0, 0), flip)
        assert sc.out_hw == tuple(want.shape[1:3]) and sc.flip is flip
        _scale_checked(sc, src, want, f"from_options {opt}")
        seen.add((crop, flip, size != p["new_size"]))
        print(f"kernels: from_options {opt['dataset_scale']} / {opt['dataset_crop']} -> {sc.out_hw} flip={flip} exact")
    assert {c for c, _, _ in seen} == {True, False} and {f for _, f, _ in seen} == {True, False} and any(q for _, _, q in seen)


def step_fullsize(dev):
    from ir2rgb_amd.transform import FrameScaler, resize_reference
    g = torch.Generator().manual_seed(11)
    src = torch.randint(0, 256, (1, 512, 640, 3), generator=g, dtype=torch.uint8)
    src[0, 100:200, 50:300] = 255            # flat saturated patches with hard edges: overshoot on both sides
    src[0, 300:420, 200:600] = 0
    for H, W in ((832, 1024), (416, 512)):
        want = resize_reference(src, (W, H))
        assert want.min() == 0 and want.max() == 255
        sc = FrameScaler(dev, (512, 640), 3, (W, H))
        _scale_checked(sc, src.to(dev), want, f"fullsize 512x640 -> {H}x{W}")
        print(f"fullsize: 512x640x3 -> {H}x{W} exact")


def _build(n_scales, ngf, seed):
    from ir2rgb_amd import networks as N
    torch.manual_seed(seed)
    gs = [N.build_generator_module(3 * TG, 3, 3 * (TG - 1), ngf, "composite", 3, "batch", 0, **G_OPT)]
    for s in range(1, n_scales):
        gs.append(N.build_generator_module(3 * TG, 3, 3 * (TG - 1), ngf // 2 ** s, "composite-local", 3, "batch", s, **G_OPT))
    return gs


def _smooth_u8(n, h, w, c, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, c, h, w, generator=g)
    x = torch.tanh(torch.nn.functional.avg_pool2d(torch.nn.functional.pad(x, (2, 2, 2, 2), mode="reflect"), 5, stride=1) * 3)
    return ((x + 1) * 127.5).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def step_translator(dev):
    from ir2rgb_amd.inference import VideoTranslator, normalise_u8
    from ir2rgb_amd.metrics import video_metrics
    from ir2rgb_amd.transform import FrameScaler, resize_reference
    H, W, hs, ws, ngf = 64, 128, 40, 72, 32
    n_seq = 6 + TG - 1
    ir_cam = _smooth_u8(2 * n_seq, hs, ws, 3, 21)
    rgb_cam = _smooth_u8(2 * n_seq, hs, ws, 3, 22)
    ir_net, rgb_net = resize_reference(ir_cam, (W, H)).to(dev), resize_reference(rgb_cam, (W, H)).to(dev)   # the host's scaling
    ir_cam, rgb_cam = ir_cam.to(dev), rgb_cam.to(dev)
    base = _build(1, ngf, 23)
    for first in ("zeros", "real"):
        results = {}
        for use_graph in (False, True):
            kw = dict(n_scales_spatial=1, first_layer_gen_filters=ngf, first_frame=first, use_graph=use_graph)
            tr_cam = VideoTranslator(dev, H, W, netG=copy.deepcopy(base), source_size=(hs, ws), **kw)
            tr_net = VideoTranslator(dev, H, W, netG=copy.deepcopy(base), **kw)
            assert tr_cam.scaler.out_hw == (H, W) and tr_net.scaler is None
            frames = []
            for k in range(2):                                          # two sequences: a reset() in between
                sl = slice(k * n_seq, (k + 1) * n_seq)
                real_cam = rgb_cam[sl] if first == "real" else None
                real_net = rgb_net[sl] if first == "real" else None
                outs_net = tr_net.translate(ir_net[sl], real_net)
                n = 0
                for a in tr_cam.translate(ir_cam[sl], real_cam):
                    b = next(outs_net)
                    assert a.shape == (H, W, 3) and torch.equal(a, b), f"{first} graph={use_graph} sequence {k} frame {n}: image"
                    for u, v in zip(tr_cam.history(), tr_net.history()):
                        assert torch.equal(u, v), f"{first} graph={use_graph} sequence {k} frame {n}: history"
                    assert torch.equal(tr_cam.hist_A[0], tr_net.hist_A[0])
                    assert torch.equal(tr_cam.stage["u8"], ir_net[sl][TG - 1 + n])      # the scaled frame itself
                    frames.append(a)
                    n += 1
                assert n == 6 and next(outs_net, None) is None
            assert len(tr_cam._graphs) == int(use_graph) and (not use_graph or "cam" in tr_cam._graphs)
            results[use_graph] = frames
            # a frame that already has the network's size is taken as before, by the same translator
            tr_cam.reset(), tr_net.reset()
            for i in range(TG):
                a = tr_cam.push(ir_net[i], rgb_net[i] if first == "real" and i < TG - 1 else None)
                b = tr_net.push(ir_net[i], rgb_net[i] if first == "real" and i < TG - 1 else None)
            assert torch.equal(a, b)
        for a, b in zip(results[False], results[True]):
            assert torch.equal(a, b), f"{first}: eager and replayed frames differ"
        print(f"translator first={first}: 2 x 6 camera-size frames = host-scaled frames, eager and graph")
    # evaluate: the targets are scaled the same way
    kw = dict(n_scales_spatial=1, first_layer_gen_filters=ngf, first_frame="zeros")
    tr_cam = VideoTranslator(dev, H, W, netG=copy.deepcopy(base), source_size=(hs, ws), **kw)
    tr_net = VideoTranslator(dev, H, W, netG=copy.deepcopy(base), **kw)
    got = tr_cam.evaluate(ir_cam[:n_seq], rgb_cam[:n_seq]).result()
    outs = torch.stack(list(tr_net.translate(ir_net[:n_seq])))
    want = torch.cat([video_metrics(rgb_net[TG - 1 + k:TG + k], outs[k:k + 1]) for k in range(6)])
    assert got["frames"] == 6 and torch.equal(got["per_frame"], want), "evaluate: rows differ from video_metrics on host-scaled targets"
    print("translator: evaluate() = video_metrics on host-scaled targets")
    # a scaler handed in: the translator works on a private clone (same tables, its own workspace), so whatever the caller
    # does with the scaler -- or with the translator's -- between replays of the captured step leaves the frames alone
    import random
    from ir2rgb_amd.frames import WindowSlicer, scaled_sequence
    sc = FrameScaler(dev, (hs, ws), 3, (W, H))
    tr_cam = VideoTranslator(dev, H, W, netG=copy.deepcopy(base), scaler=sc, use_graph=True, **kw)
    tr_net = VideoTranslator(dev, H, W, netG=copy.deepcopy(base), use_graph=True, **kw)
    assert tr_cam.scaler is not sc and tr_cam.scaler.x_tables[0] is sc.x_tables[0]
    assert tr_cam.scaler._ws.data_ptr() != sc._ws.data_ptr()
    held, junk = (tr_cam.scaler._ws.data_ptr(), sc._ws.data_ptr()), []
    outs_net = tr_net.translate(ir_net)
    for n, a in enumerate(tr_cam.translate(ir_cam)):                      # 2 * n_seq frames: replays from the third output on
        assert torch.equal(a, next(outs_net)), f"shared scaler: frame {n}"
        if n >= 3:                                                        # the 'cam' graph exists: batched calls in between
            assert "cam" in tr_cam._graphs
            big = sc(ir_cam[:5 + n % 3])
            assert torch.equal(big, ir_net[:5 + n % 3]) and torch.equal(tr_cam.scaler(rgb_cam[:4]), rgb_net[:4])
            scaled_sequence(ir_cam[:6], rgb_cam[:6], scaler=tr_cam.scaler)
            junk.append(torch.full((sc.workspace_bytes(7),), 0xEE, dtype=torch.uint8, device=dev))   # takes freed blocks
            del big
            assert (tr_cam.scaler._ws.data_ptr(), sc._ws.data_ptr()) == held
    assert n == 2 * n_seq - TG
    torch.cuda.synchronize()
    assert all(bool((j == 0xEE).all()) for j in junk), "a replay wrote into memory that a released workspace had occupied"
    print("translator: batched calls on the shared scaler between replays change nothing")
    # the scaling options: one draw per translator, applied to frames, first real frames and targets alike
    from ir2rgb_amd.transform import transform_reference
    opt = dict(dataset_scale="scale-width", dataset_crop="none", load_size=128, fine_size=64, dataset_mode="ir2rgb", is_train=True,
               flip=True)
    seed = next(s for s in range(20) if random.Random(s).random() > 0.5)      # a draw that flips
    tr_opt = VideoTranslator(dev, H, W, netG=copy.deepcopy(base), source_size=(hs, ws), scale_opt=opt,
                             scale_rng=(random.Random(seed), np.random.RandomState(seed)), **kw)
    assert tr_opt.scaler.flip and tr_opt.scaler.params["new_size"] == (W, H)
    ir_flip = transform_reference(ir_cam[:n_seq].cpu(), (W, H), flip=True).to(dev)
    assert torch.equal(ir_flip, ir_net[:n_seq].flip(2))
    for a, b in zip(tr_opt.translate(ir_cam[:n_seq]), tr_net.translate(ir_flip)):
        assert torch.equal(a, b), "scale_opt: frames differ from host-flipped frames"
    with pytest.raises(ValueError, match="the network takes"):      # 'resize' gives load_size x load_size, the network is 64 x 128
        VideoTranslator(dev, H, W, netG=copy.deepcopy(base), source_size=(hs, ws), scale_opt=dict(opt, dataset_scale="resize"), **kw)
    A, B, used = scaled_sequence(ir_cam[:5], rgb_cam[:5], rng=(random.Random(seed), np.random.RandomState(seed)), **opt)
    assert used.params == tr_opt.scaler.params and used.flip
    assert torch.equal(A.view(5, 3, H, W).cpu(), torch.stack([normalise_u8(f) for f in ir_flip[:5].cpu()]))
    print("translator: scale_opt / scale_rng and scaled_sequence(**opt) apply the drawn parameters")
    with pytest.raises(ValueError, match="the network takes"):
        VideoTranslator(dev, H, W, netG=copy.deepcopy(base), scaler=FrameScaler(dev, (hs, ws), 3, (W, H + 4)), **kw)
    with pytest.raises(ValueError):
        tr_net.push(ir_cam[0])                                          # no scaler: a camera-size frame is refused as before
    # the loader's tensors from camera-size tracks: one parameter set, one call per track
    A, B, used = scaled_sequence(ir_cam[:5], rgb_cam[:5], scaler=sc)
    assert used is sc and A.shape == (1, 15, H, W) and B.shape == (1, 15, H, W)
    # (normalise_u8 evaluated on the CPU, where torch's division is the correctly rounded one the kernel performs)
    assert torch.equal(A.view(5, 3, H, W).cpu(), torch.stack([normalise_u8(f) for f in ir_net[:5].cpu()]))
    assert torch.equal(B.view(5, 3, H, W).cpu(), torch.stack([normalise_u8(f) for f in rgb_net[:5].cpu()]))
    assert len(WindowSlicer(A, B)) == 3
    print("translator: scaled_sequence = normalise_u8 of the host-scaled tracks")


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    step = sys.argv[1]
    assert torch.cuda.is_available()
    globals()["step_" + step](torch.device("cuda:0"))
    torch.cuda.synchronize()
    print(f"step {step} ok", flush=True)
