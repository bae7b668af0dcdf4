"""Frame-by-frame inference on the GPU (ir2rgb_amd.inference, csrc/frame_io.hip).  Every step runs in a child process of
its own under its own time limit (``python tests/test_inference_gpu.py <step>``), so a step that hangs or faults ends
there and takes nothing else with it:

  kernels   the two frame-I/O kernels against the CPU restatements of tests/test_inference_cpu.py, EXACTLY (the same
            IEEE fp32 operations in the same order on both sides), canary bands around every output
  teacher   every golden case, both dtypes, every frame: the reference's own history loaded with set_history, one step,
            fake_B per scale against the reference by relative L2 <= max(1.5 x floor, floor + 0.02), floor from the file
            (teacher-forced because a random-init generator's recurrence amplifies differences)
  loop      free-running translate() over 12 frames, bit for bit against a literal restatement of generator.py:184-235
            built from avg_pool_pyramid, netG[s](...) under no_grad and torch.cat
  graph     use_graph=True against False: identical uint8 frames and histories over 12 frames across a reset()
  state     parameters and packed weights untouched by 12 frames; two translators agree
  fullsize  512x1024, two scales, bf16, six frames
"""
import copy
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


def test_frame_io_kernels_are_exact(dev):
    _run("kernels", 420)


def test_teacher_forced_frames_match_the_reference(dev):
    _run("teacher", 600)


def test_translate_is_the_literal_loop_bit_for_bit(dev):
    _run("loop", 600)


def test_graph_replay_changes_nothing(dev):
    _run("graph", 420)


def test_weights_are_untouched_and_translators_agree(dev):
    _run("state", 420)


def test_full_size_run(dev):
    _run("fullsize", 600)


# =============================================================================================
# the steps (child process)
# =============================================================================================
class Guarded:
    """A contiguous tensor inside a larger allocation whose neighbourhood holds a canary (tests/test_bounds_gpu.py)."""

    def __init__(self, init, fill):
        n = init.numel()
        self.fill = fill
        self.buf = torch.full((n + 2 * GUARD,), fill, dtype=init.dtype, device=init.device)
        self.t = self.buf[GUARD:GUARD + n].view(init.shape)
        self.t.copy_(init)

    def intact(self):
        return bool((self.buf[:GUARD] == self.fill).all() and (self.buf[-GUARD:] == self.fill).all())


def _build(n_scales, ngf, seed):
    from ir2rgb_amd import networks as N
    torch.manual_seed(seed)
    gs = [N.build_generator_module(3 * TG, 3, 3 * (TG - 1), ngf, "composite", 3, "batch", 0, **G_OPT)]
    for s in range(1, n_scales):
        gs.append(N.build_generator_module(3 * TG, 3, 3 * (TG - 1), ngf // 2 ** s, "composite-local", 3, "batch", s, **G_OPT))
    return gs


def _frames_u8(n, h, w, c, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, c, h, w, generator=g)
    x = torch.tanh(torch.nn.functional.avg_pool2d(torch.nn.functional.pad(x, (3, 3, 3, 3), mode="reflect"), 7, stride=1) * 3)
    return ((x + 1) * 127.5).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def step_kernels(dev):
    from ir2rgb_amd import autograd as A
    from ir2rgb_amd import inference as I
    from test_inference_cpu import finish_grid, finish_restatement, push_restatement, shift_restatement
    gen = torch.Generator().manual_seed(5)
    for C in (1, 3):
        for H, W in ((64, 128), (66, 130), (512, 1024)):
            Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
            for T, two_levels in ((3, True), (2, True), (3, False), (1, True)):
                frame = torch.randint(0, 256, (H, W, C), generator=gen, dtype=torch.uint8)
                want_new = push_restatement(frame)
                for src_f32 in (False, True):
                    h0 = Guarded(torch.randn(T, C, H, W, generator=gen).to(dev), 7.0)
                    h1 = Guarded(torch.randn(T, C, Ho, Wo, generator=gen).to(dev), 7.0) if two_levels else None
                    old0, old1 = h0.t.clone(), (h1.t.clone() if h1 else None)
                    src = Guarded((want_new if src_f32 else frame).to(dev), 3.0 if src_f32 else 0xA5)
                    I.frame_push(src.t, h0.t, h1.t if h1 else None)
                    torch.cuda.synchronize()
                    what = f"push C={C} {H}x{W} T={T} levels={1 + two_levels} f32={src_f32}"
                    assert torch.equal(h0.t.cpu(), shift_restatement(old0.cpu(), want_new)), what + ": full level"
                    assert h0.intact() and src.intact() and torch.equal(src.t.cpu(), want_new if src_f32 else frame), what
                    if h1:
                        pooled = A.avg_pool3s2(h0.t[-1].contiguous())          # ir2rgb_avgpool3s2 of the full level
                        assert torch.equal(h1.t[-1], pooled), what + ": pooled level differs from ir2rgb_avgpool3s2"
                        assert torch.equal(h1.t[:-1], old1[1:]), what + ": pooled history shift"
                        assert h1.intact(), what + ": wrote outside the pooled history"
    grid = finish_grid()
    for H, W in ((64, 128), (66, 130), (512, 1024)):
        for T, with_img in ((2, True), (2, False), (1, True), (4, True)):
            x = torch.randn(3, H, W, generator=gen) * 0.8
            x.view(-1)[:grid.numel()] = grid
            x.view(-1)[-grid.numel():] = grid
            gx = Guarded(x.to(dev), 3.0)
            hist = Guarded(torch.randn(T, 3, H, W, generator=gen).to(dev), 7.0)
            img = Guarded(torch.full((H, W, 3), 9, dtype=torch.uint8, device=dev), 0xA5)
            old = hist.t.clone()
            I.frame_finish(gx.t, hist.t, img.t if with_img else None)
            torch.cuda.synchronize()
            what = f"finish {H}x{W} T={T} img={with_img}"
            assert torch.equal(hist.t.cpu(), shift_restatement(old.cpu(), x)), what + ": history"
            if with_img:
                assert np.array_equal(img.t.cpu().numpy(), finish_restatement(x)), what + ": uint8 image"
            else:
                assert bool((img.t == 9).all())
            assert hist.intact() and img.intact() and gx.intact() and torch.equal(gx.t.cpu(), x), what + ": canary"
    print("kernels: all push / finish forms exact")


def _bound(floor):
    return max(1.5 * floor, floor + 0.02)


def step_teacher(dev):
    import importlib.util
    from ir2rgb_amd.inference import VideoTranslator
    from test_inference_cpu import CASES
    spec = importlib.util.spec_from_file_location("make_infer_goldens", os.path.join(GOLDEN, "make_infer_goldens.py"))
    M = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(M)
    worst = 0.0
    for tag in CASES:
        d = np.load(os.path.join(GOLDEN, f"infer_{tag}.npz"))
        ns, ngf, seed, first, ev = int(d["n_scales"]), int(d["ngf"]), int(d["seed"]), str(d["first_frame"]), bool(d["eval_mode"])
        ir = torch.as_tensor(d["ir_u8"]).to(dev)
        rgb = torch.as_tensor(d["rgb_u8"]).to(dev) if first == "real" else None
        for name, dt in (("bf16", torch.bfloat16), ("f16", torch.float16)):
            netG = _build(ns, ngf, seed)
            kw = dict(netG=netG, n_scales_spatial=ns, first_layer_gen_filters=ngf, first_frame=first, compute_dtype=dt,
                      use_graph=False)
            if ev:      # the golden's running statistics: three training-mode forwards of windows 0..2 from the first history
                warm = VideoTranslator(dev, 64, 128, norm_stats="batch", **kw)
                for k in range(int(d["eval_warm_forwards"])):
                    warm.reset()
                    for j in range(TG - 1):
                        warm.push(ir[k + j], rgb[j])
                    warm.set_history([h.to(dev) for h in M.history(d, 0)])
                    warm.push(ir[k + TG - 1])
            tr = VideoTranslator(dev, 64, 128, norm_stats="running" if ev else "batch", **kw)
            for t in range(d["tf/s0"].shape[0]):
                tr.reset()
                for j in range(TG - 1):
                    assert tr.push(ir[t + j], rgb[j] if rgb is not None else None) is None
                if not (t == 0 and first == "zeros"):       # frame 0 of no_first_img is the first-frame path itself
                    tr.set_history([h.to(dev) for h in M.history(d, t)])
                out = tr.push(ir[t + TG - 1])
                assert out.dtype == torch.uint8 and out.shape == (64, 128, 3)
                for i in range(ns):
                    want = torch.as_tensor(d[f"tf/s{i}"][t]).float()
                    got = tr.hist_B[i][-1].cpu()
                    rel = ((got - want).norm() / want.norm()).item()
                    floor = float(d[f"floor/{name}/s{i}"][t])
                    print(f"teacher {tag} {name} frame {t} scale {i}: rel L2 {rel:.5f}  floor {floor:.5f}  bound {_bound(floor):.5f}")
                    assert torch.isfinite(got).all()
                    assert rel <= _bound(floor), (tag, name, t, i, rel, floor)
                    worst = max(worst, rel / _bound(floor))
    print(f"teacher: worst rel / bound = {worst:.3f}")


def literal_loop(netG, A_all, real_B, first_frame, n_scales):
    """generator.py:184-235 + test_vid2vid.py:36-46 from parts that exist without ir2rgb_amd.inference: -> fake_B per
    frame, full resolution.  ``A_all`` [1,N,C,H,W], ``real_B`` [1,tG-1,3,H,W] or None, both fp32 on the device."""
    from ir2rgb_amd.vid2vid import avg_pool_pyramid
    outs, fake_B_prev = [], None
    no_first_img = first_frame == "zeros"
    with torch.no_grad():
        for t in range(A_all.shape[1] - TG + 1):
            real_A = A_all[:, t:t + TG]
            is_first_frame = fake_B_prev is None
            if is_first_frame:                                              # generate_first_frame
                prev = torch.zeros_like(A_all[:, :TG - 1, :3]) if no_first_img else real_B[:, :TG - 1]
                fake_B_prev = [B[0] for B in avg_pool_pyramid(prev.contiguous(), n_scales)]
            real_A = avg_pool_pyramid(real_A.contiguous(), n_scales)
            fake_B_feat = flow_feat = None
            for s in range(n_scales):                                       # generate_frame_infer
                si = n_scales - 1 - s
                _, _, _, h, w = real_A[si].shape
                out = netG[s](real_A[si][0, :TG].reshape(1, -1, h, w), fake_B_prev[si].reshape(1, -1, h, w), None, fake_B_feat,
                              flow_feat, None, no_first_img and is_first_frame)
                fake_B, fake_B_feat, flow_feat = out[0], out[4], out[5]
                fake_B_prev[si] = torch.cat([fake_B_prev[si][1:], fake_B])
            outs.append(fake_B[0].clone())
    return outs


def _inputs(dev, n_frames, h, w, seed):
    from test_inference_cpu import push_restatement
    ir = _frames_u8(n_frames, h, w, 3, seed)
    rgb = _frames_u8(TG - 1, h, w, 3, seed + 1)
    A_all = torch.stack([push_restatement(f) for f in ir]).unsqueeze(0).to(dev)
    real_B = torch.stack([push_restatement(f) for f in rgb]).unsqueeze(0).to(dev)
    return ir.to(dev), rgb.to(dev), A_all, real_B


def step_loop(dev):
    from ir2rgb_amd.inference import VideoTranslator, to_u8
    ir, rgb, A_all, real_B = _inputs(dev, 12 + TG - 1, 64, 128, 40)
    for ns, ngf in ((1, 64), (2, 64)):
        base = _build(ns, ngf, 50 + ns)
        for first in ("zeros", "real"):
            for norm in ("batch", "running"):
                ref_G = [g.to(dev).train(norm == "batch") for g in copy.deepcopy(base)]
                for g in ref_G:
                    g.compute_dtype = torch.bfloat16
                want = literal_loop(ref_G, A_all, real_B, first, ns)
                tr = VideoTranslator(dev, 64, 128, netG=copy.deepcopy(base), n_scales_spatial=ns, first_layer_gen_filters=ngf,
                                     first_frame=first, norm_stats=norm)
                tr.reset()
                n = 0
                for i in range(ir.shape[0]):
                    out = tr.push(ir[i], rgb[i] if (first == "real" and i < TG - 1) else None)
                    if out is None:
                        assert i < TG - 1
                        continue
                    got = tr.hist_B[0][-1]
                    assert torch.equal(got, want[n]), f"loop ns={ns} first={first} norm={norm}: frame {n} differs " \
                        f"(max |d| {(got - want[n]).abs().max().item():.3e})"
                    assert torch.equal(out, to_u8(want[n]))
                    n += 1
                assert n == 12 and len(tr._graphs) == 1
                if norm == "batch":     # the running statistics advanced exactly as the literal loop's did
                    for a, b in zip(tr.netG, ref_G):
                        for (k, u), (_, v) in zip(a.state_dict().items(), b.state_dict().items()):
                            assert torch.equal(u, v), k
                print(f"loop ns={ns} first={first} norm={norm}: 12 frames bit-identical")
    # the reference-shaped call gives the same frames
    base = _build(2, 64, 52)
    want = literal_loop([g.to(dev).train() for g in copy.deepcopy(base)], A_all, real_B, "real", 2)
    tr = VideoTranslator(dev, 64, 128, netG=copy.deepcopy(base), n_scales_spatial=2, first_layer_gen_filters=64, first_frame="real")
    for t in range(6):
        fake_B, last_A = tr.inference(A_all[:, t:t + TG].cpu(), real_B.cpu() if t == 0 else None)
        assert torch.equal(fake_B, want[t]) and torch.equal(last_A, A_all[0, t + TG - 1])
    print("loop: inference() agrees")


def step_graph(dev):
    from ir2rgb_amd.inference import VideoTranslator
    ir, rgb, _, _ = _inputs(dev, 12 + 2 * (TG - 1), 64, 128, 60)
    for ns, ngf, first in ((2, 64, "zeros"), (1, 64, "real")):
        base = _build(ns, ngf, 70 + ns)
        runs = []
        for use_graph in (False, True):
            tr = VideoTranslator(dev, 64, 128, netG=copy.deepcopy(base), n_scales_spatial=ns, first_layer_gen_filters=ngf,
                                 first_frame=first, use_graph=use_graph)
            frames, hists = [], []
            for part in (ir[:8], ir[8:]):                   # two sequences of 6 frames: a reset() in the middle
                for out in tr.translate(part, rgb if first == "real" else None):
                    frames.append(out)
                    hists.append(tr.history())
            assert len(frames) == 12 and len(tr._graphs) == int(use_graph)
            runs.append((frames, hists))
        for n in range(12):
            assert torch.equal(runs[0][0][n], runs[1][0][n]), f"graph ns={ns}: uint8 frame {n} differs"
            for a, b in zip(runs[0][1][n], runs[1][1][n]):
                assert torch.equal(a, b), f"graph ns={ns}: history after frame {n} differs"
        assert len({f.data_ptr() for f in runs[1][0]}) == 12          # returned frames are the caller's own
        print(f"graph ns={ns} first={first}: 12 frames and histories identical, eager vs replay")


def _packed(netG):
    out = {}
    for s, g in enumerate(netG):
        for name, m in g.named_modules():
            for tag, hit in m.__dict__.get("_ir2rgb_packed", {}).items():
                for j, t in enumerate(hit):
                    if isinstance(t, torch.Tensor):
                        out[(s, name, tag, j)] = t
    return out


def step_state(dev):
    from ir2rgb_amd.inference import VideoTranslator
    ir, rgb, _, _ = _inputs(dev, 12 + TG - 1, 64, 128, 80)
    netG = _build(2, 64, 81)
    kw = dict(netG=netG, n_scales_spatial=2, first_layer_gen_filters=64, first_frame="zeros")
    tr = VideoTranslator(dev, 64, 128, **kw)
    list(tr.translate(ir[:4]))                                              # the packed copies exist from here on
    params = {(s, k): p.detach().clone() for s, g in enumerate(netG) for k, p in g.named_parameters()}
    packed = {k: t.clone() for k, t in _packed(netG).items()}
    assert len(packed) > 50
    first_run = list(tr.translate(ir))
    assert len(first_run) == 12
    for (s, k), p in params.items():
        q = dict(netG[s].named_parameters())[k]
        assert torch.equal(p, q) and q.grad is None, k
    now = _packed(netG)
    assert set(now) == set(packed)
    for k, t in packed.items():
        assert torch.equal(t, now[k]), k
    second = VideoTranslator(dev, 64, 128, **kw)                            # same weights, same frames
    for a, b in zip(first_run, second.translate(ir)):
        assert torch.equal(a, b)
    print("state: parameters and", len(packed), "packed buffers untouched; two translators agree")


def step_fullsize(dev):
    from ir2rgb_amd import inference as I
    H, W = 512, 1024
    ir = _frames_u8(6 + TG - 1, H, W, 3, 90).to(dev)
    tr = I.VideoTranslator(dev, H, W, netG=_build(2, 128, 91), n_scales_spatial=2, first_layer_gen_filters=128,
                           first_frame="zeros", compute_dtype=torch.bfloat16)
    # canary bands around the static buffers the graph writes
    for name in ("hist_A", "hist_B"):
        setattr(tr, "_g_" + name, [Guarded(t, 7.0) for t in getattr(tr, name)])
        setattr(tr, name, [g.t for g in getattr(tr, "_g_" + name)])
    g_img = Guarded(tr.image, 0xA5)
    tr.image = g_img.t
    n = 0
    for out in tr.translate(ir):
        fake_B = tr.hist_B[0][-1]
        assert torch.isfinite(fake_B).all() and fake_B.abs().max() <= 1.0 + 1e-5
        assert torch.equal(out, I.to_u8(fake_B)) and out.shape == (H, W, 3)
        n += 1
    torch.cuda.synchronize()
    assert n == 6 and len(tr._graphs) == 1
    assert all(g.intact() for g in tr._g_hist_A + tr._g_hist_B) and g_img.intact()
    print("fullsize: six 512x1024 frames, finite, uint8 = restatement, canaries intact")


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    step = sys.argv[1]
    assert torch.cuda.is_available()
    globals()["step_" + step](torch.device("cuda:0"))
    torch.cuda.synchronize()
    print(f"step {step} ok", flush=True)
