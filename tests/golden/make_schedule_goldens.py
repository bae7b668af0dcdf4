"""Generates tests/golden/window_2scale_fixglobal_ngf64_64x128.npz: training windows of the epochs in which only the
finest spatial scale trains (``--niter_fix_global``), from the REFERENCE's own code.

Everything is tests/golden/make_window_goldens.py's (same imports from the reference, same restated wrappers, same
loop body, same rounding-floor twins); this file adds the two places where the reference's generator branches on
``finetune_all``:

    generator.py:64-72     optimizer_G over the finest scale's parameters alone
    generator.py:166-170   the coarser scales' fake_B / feature / flow / flow-feature outputs detached

Two windows at 64x128, two spatial scales, ngf 64 -> 32.  Records as ``window_case`` writes them (loss terms and outputs
per window, window-0 gradients, ``floor/...`` distances to the rounding-emulating twins, a few tensors after the Adam
steps), with two differences that keep the file small: the input sequences are rounded to f16 before anything runs and
stored as f16, and of the discriminator's gradients only the norms and the small tensors are stored.  While
generating, the coarse generator's parameters are asserted to have no gradient and to be bit-unchanged after both
windows.

    python tests/golden/make_schedule_goldens.py
"""
import copy
import os

import numpy as np
import torch

import make_window_goldens as W
from make_window_goldens import BASE_OPT, D_KEEP, G_KEEP, OUT, RefModelD, RefModelG, concat, run_windows
from window_stub import smooth

TAG = "2scale_fixglobal_ngf64_64x128"
D_KEEP_SMALL = tuple(k for k in D_KEEP if k != "scale1_layer1.0.weight")       # (that one alone is 512 KiB)


class FixGlobalModelG(RefModelG):
    """RefModelG with ``niter_fix_global != 0``: generator.py:64-72 and :166-170."""

    def __init__(self, opt, seed):
        super().__init__(opt, seed)
        self.finetune_all = False                                            # generator.py:64 (niter_fix_global != 0)
        self.set_optimizer()

    def set_optimizer(self):
        params = list(self.netG[self.n_scales - 1].parameters())             # generator.py:69
        if self.finetune_all:                                                # generator.py:70-72
            for s in range(self.n_scales - 1):
                params += list(self.netG[s].parameters())
        self.optimizer_G = torch.optim.Adam(params, lr=self.opt["lr"], betas=(self.opt["beta1"], 0.999))

    def generate_frame_train(self, real_A_all, fake_B_pyr, is_first_frame):   # generator.py:125-182
        tG, n_scales = self.opt["n_input_gen_frames"], self.n_scales
        finetune_all = self.finetune_all
        real_A_pyr = W.build_pyr(real_A_all, n_scales)
        fake_Bs_raw, flows, weights = None, None, None
        for t in range(self.n_frames_load):
            fake_B_feat = flow_feat = None
            for s in range(n_scales):
                si = n_scales - 1 - s
                real_As = real_A_pyr[si]
                _, _, _, h, w = real_As.size()
                real_As_reshaped = real_As[:, t:t + tG, ...].reshape(self.bs, -1, h, w)
                fake_B_prevs = fake_B_pyr[si][:, t:t + tG - 1, ...]
                if (t % self.n_frames_bp) == 0:
                    fake_B_prevs = fake_B_prevs.detach()
                fake_B_prevs_reshaped = fake_B_prevs.reshape(self.bs, -1, h, w)
                use_raw_only = self.opt["no_first_img"] and is_first_frame
                fake_B, flow, weight, fake_B_raw, fake_B_feat, flow_feat = self._net(
                    s, real_As_reshaped, fake_B_prevs_reshaped, fake_B_feat, flow_feat, use_raw_only)
                if s != n_scales - 1 and not finetune_all:                   # generator.py:166-170
                    fake_B, fake_B_feat = fake_B.detach(), fake_B_feat.detach()
                    if flow is not None:
                        flow, flow_feat = flow.detach(), flow_feat.detach()
                fake_B_pyr[si] = concat([fake_B_pyr[si], fake_B.unsqueeze(1)], dim=1)
                if s == n_scales - 1:
                    fake_Bs_raw = concat([fake_Bs_raw, fake_B_raw.unsqueeze(1)], dim=1)
                    if flow is not None:
                        flows = concat([flows, flow.unsqueeze(1)], dim=1)
                        weights = concat([weights, weight.unsqueeze(1)], dim=1)
        return fake_B_pyr, fake_Bs_raw, flows, weights


def fixglobal_case(tag=TAG, n_windows=2, H=64, Wd=128, ngf=64, seed=131, lr=2e-4, floor_windows=2):
    opt = dict(BASE_OPT, n_scales_spatial=2, first_layer_gen_filters=ngf, lr=lr)
    model_g = FixGlobalModelG(opt, seed)
    model_d = RefModelD(opt, seeds=(seed + 1, seed + 2))
    tG = opt["n_input_gen_frames"]
    n_frames = n_windows + tG - 1
    seq_A = smooth((1, n_frames, 3, H, Wd), seed + 5).half().float()          # (exact in f16: stored as such)
    seq_B = smooth((1, n_frames, 3, H, Wd), seed + 6).half().float()
    out = {"seq_A": seq_A.numpy().astype(np.float16), "seq_B": seq_B.numpy().astype(np.float16)}
    coarse0 = {k: v.clone() for k, v in model_g.netG[0].named_parameters()}
    buffers0 = {k: v.clone() for k, v in model_g.netG[0].named_buffers()}
    twins = {}
    for name, dt in (("f16", torch.float16), ("bf16", torch.bfloat16)):     # copies made before anything is stepped
        tg, td = FixGlobalModelG.__new__(FixGlobalModelG), RefModelD.__new__(RefModelD)
        tg.__dict__.update({k: v for k, v in model_g.__dict__.items() if k not in ("netG", "optimizer_G")})
        td.__dict__.update({k: v for k, v in model_d.__dict__.items() if k not in ("netD", "netD_T", "optimizer_D", "optimizer_D_T")})
        tg.netG = copy.deepcopy(model_g.netG)
        td.netD, td.netD_T = copy.deepcopy(model_d.netD), copy.deepcopy(model_d.netD_T)
        adam = dict(lr=opt["lr"], betas=(opt["beta1"], 0.999))
        tg.set_optimizer()
        td.optimizer_D = torch.optim.Adam(list(td.netD.parameters()), **adam)
        td.optimizer_D_T = [torch.optim.Adam(list(d.parameters()), **adam) for d in td.netD_T]
        tg.emulate = td.emulate = dt
        twins[name] = (tg, td)
    recs, grads = run_windows(model_g, model_d, seq_A, seq_B, n_windows, opt, tag=tag)
    # the coarse generator: no gradient, not one bit of its parameters moved, its running statistics did
    for k, p in model_g.netG[0].named_parameters():
        assert p.grad is None, f"coarse parameter {k} received a gradient"
        assert torch.equal(p, coarse0[k]), f"coarse parameter {k} changed"
    assert grads["G0"] == {}
    assert any(not torch.equal(v, buffers0[k]) for k, v in model_g.netG[0].named_buffers() if "running" in k)
    for i, (rec, outs) in enumerate(recs):
        out.update({f"w{i}/loss/{k}": np.float64(v) for k, v in rec.items()})
        out.update({f"w{i}/{k}": v.numpy().astype(np.float16) for k, v in outs.items()})
    for s, g in enumerate(model_g.netG):
        norms = {k: grads[f"G{s}"][k].double().norm().item() if k in grads[f"G{s}"] else 0.0 for k, _ in g.named_parameters()}
        out[f"w0/G{s}/grad_names"], out[f"w0/G{s}/grad_norms"] = np.array(list(norms)), np.array(list(norms.values()))
        out.update({f"w0/G{s}/grad/{k}": grads[f"G{s}"][k].numpy() for k in G_KEEP if k in grads[f"G{s}"]})
    norms = {k: grads["D"][k].double().norm().item() if k in grads["D"] else 0.0 for k, _ in model_d.netD.named_parameters()}
    out["w0/D/grad_names"], out["w0/D/grad_norms"] = np.array(list(norms)), np.array(list(norms.values()))
    out.update({f"w0/D/grad/{k}": grads["D"][k].numpy() for k in D_KEEP_SMALL if k in grads["D"]})
    # the rounding floor (window_case's records; the coarse generator has no gradients to compare)
    for name, (tg, td) in twins.items():
        erecs, egrads = run_windows(tg, td, seq_A, seq_B, floor_windows, opt, tag=f"{tag} emulated {name}")
        assert egrads["G0"] == {}
        fl = {}
        for i in range(floor_windows):
            for k, v in erecs[i][0].items():
                fl[f"floor/{name}/w{i}/loss/{k}"] = abs(v - recs[i][0][k]) / max(abs(recs[i][0][k]), 0.05)
            for k, v in erecs[i][1].items():
                fl[f"floor/{name}/w{i}/out/{k}"] = ((v - recs[i][1][k]).norm() / recs[i][1][k].norm()).item()
        for prefix, keep in [("G1", G_KEEP), ("D", D_KEEP_SMALL)]:
            got, want = egrads[prefix], grads[prefix]
            for k in keep:
                if k in want and k in got and want[k].norm() > 0:
                    a, b = got[k].double().flatten(), want[k].double().flatten()
                    fl[f"floor/{name}/{prefix}/l2/{k}"] = ((a - b).norm() / b.norm()).item()
                    fl[f"floor/{name}/{prefix}/proj/{k}"] = abs((a @ b / (b @ b)).item() - 1.0)
            tot_a = torch.sqrt(sum(v.double().pow(2).sum() for v in got.values()))
            tot_b = torch.sqrt(sum(v.double().pow(2).sum() for v in want.values()))
            fl[f"floor/{name}/{prefix}/total_norm"] = abs(tot_a / tot_b - 1).item()
        print("rounding floor", tag, name, {k.split("/", 2)[2]: round(v, 4) for k, v in fl.items() if "/out/" in k or "/loss/G" in k},
              flush=True)
        out.update({k: np.float64(v) for k, v in fl.items()})
    sd = model_g.netG[-1].state_dict()
    for k in ("model_final_img.1.weight", "model_final_img.1.bias", "model_down_seg.2.weight"):
        out[f"after/G/{k}"] = sd[k].numpy().copy()
    sd = model_d.netD.state_dict()
    for k in ("scale0_layer0.0.bias", "scale1_layer4.0.weight"):
        out[f"after/D/{k}"] = sd[k].numpy().copy()
    path = os.path.join(OUT, f"window_{tag}.npz")
    W.savez_fixed(path, seed=np.int64(seed), n_windows=np.int64(n_windows), ngf=np.int64(ngf), lr=np.float64(lr),
                  floor_windows=np.int64(floor_windows), no_first_img=np.bool_(False), n_scales_spatial=np.int64(2),
                  niter_fix_global=np.int64(1), **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    torch.set_num_threads(8)
    fixglobal_case()
    print("ok")
