"""Generates the inference goldens tests/golden/infer_*.npz from the REFERENCE's own generator modules.

Imported from /root/reference (importable in the authoring container; never travels to the GPU box):

    models.networks     build_generator_module, get_grid                                   (networks.py:15-82)

``models.generator`` itself is not importable (it pulls in cv2 through util/util.py), so, as
tests/golden/make_window_goldens.py does for the training path, the statements of

    Vid2VidGenerator.inference / generate_frame_infer / generate_first_frame   generator.py:184-235
    Model.build_pyr                                                            base_model.py:64-82
    ToTensor + Normalize(0.5, 0.5)                                             data/transform.py:82-85

are executed here around the reference's modules, each block citing the lines it follows.  The module's own warp calls
``.cuda()`` (networks.py:93-100): the module runs with use_raw_only=True and the blend of networks.py:207-209 / :305-307
is applied outside with the same arithmetic (as make_window_goldens.RefModelG._net).  CPU, fp32, seeded init; the
weights are never stored (ir2rgb_amd.networks builds bit-identical ones from the same seed, asserted here).

Per case, eight input frames at 64x128 (tG = 3: six generated frames):

    ir_u8                       the input frames, uint8 [8,H,W,3]
    rgb_u8                      the first tG-1 real RGB frames, uint8 (first_frame="real" cases)
    free/s{i}  [6,3,h,w] f16    the free-running fp32 loop's fake_B per pyramid level i (0 = full resolution)
    tf/s{i}    [6,3,h,w] f16    the teacher-forced frames: frame t generated from the STORED history of frame t
    floor/{bf16,f16}/s{i} [6]   the rounding floor: the teacher-forced step through oracle/emulated.py (values rounded where
                                the HIP path stores a half tensor) against the fp32 step, relative L2 per frame

The generated-frame history that went into frame t is, per level, ``free/s{i}[t-2:t]`` (the two frames generated before
it) and for t < 2 the first-frame rule (zeros, or the pyramid of the normalised ``rgb_u8``) -- ``history(npz, t)`` below
is the one definition of that, used by this script and by the tests.  Because it is stored in float16, the teacher-forced
frames are generated from exactly the stored values: ``tf`` differs from ``free`` only through the rounding of the
history (frame 0, whose history is exact, is identical).

The ``_eval`` case puts the modules in ``.eval()`` after a few training-mode forwards have moved the running statistics.
oracle/emulated.py restates training-mode BatchNorm only; for this case its ``conv_stage`` is replaced, here, by the
frozen-statistics form of the same rounding points (convolution output without bias rounded to half, then
y * scale + shift with scale = gamma * rsqrt(running_var + eps), shift = beta - (running_mean - conv_bias) * scale:
ir2rgb_bn_finalize_ex(frozen) of include/ir2rgb_hip.h).

    python tests/golden/make_infer_goldens.py
"""
import io
import os
import sys
import zipfile

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.dirname(os.path.abspath(__file__))
G_OPT = dict(gen_blocks=9, n_blocks_local=3, fg=False, no_flow=False, n_local_enhancers=1, feat_num=3)
TG, H, W, N_FRAMES = 3, 64, 128, 8

CASES = {
    # tag: (n_scales, ngf of the coarsest generator, first_frame, eval mode, seed)
    "1scale_ngf64_zeros": (1, 64, "zeros", False, 190),
    "2scale_ngf128_real": (2, 128, "real", False, 197),
    "2scale_ngf128_real_eval": (2, 128, "real", True, 197),
}


def normalise_u8(frame_u8):
    """ToTensor + Normalize(0.5, 0.5) (data/transform.py:82-85): uint8 [...,H,W,C] -> fp32 [...,C,H,W]."""
    x = torch.as_tensor(frame_u8).movedim(-1, -3).contiguous().float().div(255)
    return x.sub(0.5).div(0.5)


def build_pyr(tensor, n_scales):                                            # base_model.py:64-82
    tensor = [tensor]
    downsample = torch.nn.AvgPool2d(3, stride=2, padding=[1, 1], count_include_pad=False)
    for s in range(1, n_scales):
        b, t, c, h, w = tensor[-1].size()
        down = downsample(tensor[-1].view(-1, h, w)).view(b, t, c, h // 2, w // 2)
        tensor.append(down)
    return tensor


def first_history(npz, n_scales):
    """generate_first_frame (generator.py:217-235): the pyramid of zeros (no_first_img) or of the given real frames."""
    if str(npz["first_frame"]) == "zeros":
        prev = torch.zeros(1, TG - 1, 3, H, W)
    else:
        prev = normalise_u8(npz["rgb_u8"]).unsqueeze(0)[:, :TG - 1]
    return [B[0] for B in build_pyr(prev, n_scales)]


def history(npz, t):
    """The generated-frame history that goes into frame t, per pyramid level: fp32 [tG-1,3,h,w], oldest first."""
    n_scales = int(npz["n_scales"])
    hist = first_history(npz, n_scales)
    for i in range(n_scales):
        frames = torch.as_tensor(np.asarray(npz[f"free/s{i}"])).float()
        hist[i] = torch.cat([hist[i], frames[:t]])[t:t + TG - 1]
    return hist


def main():
    sys.dont_write_bytecode = True
    sys.path.insert(0, ROOT)
    sys.path.insert(0, "/root/reference")
    from models import networks as ref           # noqa: E402  (the reference)
    from ir2rgb_amd import networks as mine      # noqa: E402
    from oracle import emulated                  # noqa: E402
    sys.path.insert(0, OUT)
    from window_stub import smooth               # noqa: E402

    def build(mod, n_scales, ngf, seed):
        torch.manual_seed(seed)
        gs = [mod.build_generator_module(3 * TG, 3, 3 * (TG - 1), ngf, "composite", 3, "batch", 0, **G_OPT)]
        for s in range(1, n_scales):
            gs.append(mod.build_generator_module(3 * TG, 3, 3 * (TG - 1), ngf // 2 ** s, "composite-local", 3, "batch", s, **G_OPT))
        return gs

    def blend(raw, flow, weight, prev):                                     # networks.py:93-100, :207-209 / :305-307
        b, _, h, w = raw.shape
        grid = ref.get_grid(b, h, w, device="cpu", dtype=flow.dtype)
        fl = torch.cat([flow[:, 0:1] / ((w - 1.0) / 2.0), flow[:, 1:2] / ((h - 1.0) / 2.0)], dim=1)
        warp = F.grid_sample(prev[:, -3:], (grid + fl).permute(0, 2, 3, 1), mode="bilinear", padding_mode="border")
        return raw * weight + warp * (1 - weight)

    # ---- the frozen-statistics form of emulated.conv_stage (see the module docstring) ----
    train_conv_stage = emulated.conv_stage

    def conv_stage_any(x, conv, bn, act, dt, pad_reflect=0, res=(), training=True):
        if bn is None or bn.training:
            return train_conv_stage(x, conv, bn, act, dt, pad_reflect, res, training)
        if pad_reflect:
            x = F.pad(x, (pad_reflect,) * 4, mode="reflect")
        w = emulated.rste(conv.weight, dt)
        if isinstance(conv, nn.ConvTranspose2d):
            y32 = F.conv_transpose2d(x, w, None, conv.stride, conv.padding, conv.output_padding)
        else:
            y32 = F.conv2d(x, w, None, conv.stride, conv.padding if not pad_reflect else 0)
        scale = bn.weight * torch.rsqrt(bn.running_var + bn.eps)
        shift = bn.bias - (bn.running_mean - conv.bias) * scale
        z = emulated.rfb(y32, dt) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
        if act is not None:
            z = emulated._act(z, act)
        for r in res:
            if r is not None:
                z = z + r
        return emulated.rfb(z, dt)

    emulated.conv_stage = conv_stage_any

    def frame(netG, real_A, fake_B_prev, is_first, no_first_img, emulate=None):
        """inference (generator.py:191-195) + generate_frame_infer (:197-215) for one frame; ``fake_B_prev`` is updated in
        place as the reference's attribute is.  -> fake_B per scale index si."""
        n_scales = len(netG)
        real_A = build_pyr(real_A, n_scales)
        fake_B_feat = flow_feat = None
        outs = [None] * n_scales
        for s in range(n_scales):
            ra = real_A[n_scales - 1 - s]
            _, _, _, h, w = ra.size()
            si = n_scales - 1 - s
            real_As_reshaped = ra[0, :TG].view(1, -1, h, w)
            fake_B_prevs_reshaped = fake_B_prev[si].view(1, -1, h, w)
            use_raw_only = no_first_img and is_first
            if emulate is None:
                _, flow, weight, raw, fake_B_feat, flow_feat, _ = netG[s].forward(
                    real_As_reshaped, fake_B_prevs_reshaped, None, fake_B_feat, flow_feat, None, True)
            else:
                _, flow, weight, raw, fake_B_feat, flow_feat, _ = emulated.generator_forward(
                    netG[s], real_As_reshaped, fake_B_prevs_reshaped, fake_B_feat, flow_feat, True, dtype=emulate)
            fake_B = raw if use_raw_only else blend(raw, flow, weight, fake_B_prevs_reshaped)
            fake_B_prev[si] = torch.cat([fake_B_prev[si][1:, ...], fake_B])
            outs[si] = fake_B[0]
        return outs

    for tag, (n_scales, ngf, first_frame, eval_mode, seed) in CASES.items():
        netG = build(ref, n_scales, ngf, seed)
        for a, b in zip(netG, build(mine, n_scales, ngf, seed)):
            sa, sb = a.state_dict(), b.state_dict()
            assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa), "init differs"
        ir_u8 = ((smooth((N_FRAMES, 3, H, W), seed + 5) + 1) * 127.5).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
        rgb_u8 = ((smooth((TG - 1, 3, H, W), seed + 6) + 1) * 127.5).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
        out = {"n_scales": np.int64(n_scales), "ngf": np.int64(ngf), "seed": np.int64(seed), "first_frame": np.array(first_frame),
               "eval_mode": np.bool_(eval_mode), "ir_u8": ir_u8.numpy()}
        if first_frame == "real":
            out["rgb_u8"] = rgb_u8.numpy()
        A_all = normalise_u8(ir_u8).unsqueeze(0)                            # [1,8,3,H,W]
        no_first_img = first_frame == "zeros"
        with torch.no_grad():
            if eval_mode:
                # running statistics away from their initial (0, 1): three training-mode forwards (windows 0..2, first-frame history)
                warm = first_history(out, n_scales)
                for k in range(3):
                    frame(netG, A_all[:, k:k + TG], [h.clone() for h in warm], False, False)
                for g in netG:
                    g.eval()
                out["eval_warm_forwards"] = np.int64(3)
            # ---- free-running loop (test_vid2vid.py:36-46 with the window sliding by one frame)
            n_gen = N_FRAMES - TG + 1
            fake_B_prev = first_history(out, n_scales)
            free = [[] for _ in range(n_scales)]
            for t in range(n_gen):
                fb = frame(netG, A_all[:, t:t + TG], fake_B_prev, t == 0, no_first_img)
                for i in range(n_scales):
                    free[i].append(fb[i])
            for i in range(n_scales):
                out[f"free/s{i}"] = torch.stack(free[i]).numpy().astype(np.float16)
            # ---- teacher-forced frames from the stored history, and the rounding floor of each
            tf = [[] for _ in range(n_scales)]
            floors = {name: [[] for _ in range(n_scales)] for name in ("bf16", "f16")}
            for t in range(n_gen):
                hist = history(out, t)
                fb = frame(netG, A_all[:, t:t + TG], [h.clone() for h in hist], t == 0, no_first_img)
                for i in range(n_scales):
                    tf[i].append(fb[i])
                for name, dt in (("bf16", torch.bfloat16), ("f16", torch.float16)):
                    eb = frame(netG, A_all[:, t:t + TG], [h.clone() for h in hist], t == 0, no_first_img, emulate=dt)
                    for i in range(n_scales):
                        floors[name][i].append(((eb[i] - fb[i]).norm() / fb[i].norm()).item())
            for i in range(n_scales):
                out[f"tf/s{i}"] = torch.stack(tf[i]).numpy().astype(np.float16)
                for name in floors:
                    out[f"floor/{name}/s{i}"] = np.array(floors[name][i], dtype=np.float64)
        print(tag, {k: np.round(v, 4).tolist() for k, v in out.items() if k.startswith("floor/")}, flush=True)
        path = os.path.join(OUT, f"infer_{tag}.npz")
        with zipfile.ZipFile(path, "w") as z:                                # fixed timestamps: a second run is byte-identical
            for k, v in out.items():
                buf = io.BytesIO()
                np.save(buf, np.asarray(v), allow_pickle=False)
                info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
                info.compress_type = zipfile.ZIP_DEFLATED
                z.writestr(info, buf.getvalue())
        print(tag, "->", path, os.path.getsize(path), "bytes", flush=True)


if __name__ == "__main__":
    main()
