"""Frames per second of frame-by-frame inference at 512x1024, bf16: one scale (ngf 128) and two scales (ngf 128 / 64, the
bench.py configuration), 50 frames after warm-up, three ways on the same weights and the same device-resident frames:

  (a) literal   the loop of generator.py:184-235 from avg_pool_pyramid, netG[s](...) under no_grad and torch.cat, plus
                util.tensor2im's expression in numpy on the host -- what the job costs without ir2rgb_amd.inference
  (b) eager     VideoTranslator(use_graph=False)
  (c) graph     VideoTranslator(use_graph=True): one HIP-graph replay per frame

Each figure: device events around the 50 frames and one synchronise; the three ways alternate over ``--rounds`` rounds and
the median round is reported (frames/s, ms/frame).  The two frame-I/O kernels, the scores of one frame
(ir2rgb_amd.metrics.video_metrics, colour_metrics) and the two passes of frame scaling (ir2rgb_amd.transform.FrameScaler, 512x640x3 ->
832x1024 and -> 416x512) are timed alone beside the bytes they move (computed from the shapes).  Needs the GPU;
prints one JSON document and writes it to ``--out``.

    python tools/bench_infer.py --out profiles/inference_512x1024.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TG = 3
G_OPT = dict(gen_blocks=9, n_blocks_local=3, fg=False, no_flow=False, n_local_enhancers=1, feat_num=3)


def build(n_scales, ngf, dev):
    from ir2rgb_amd import networks as N
    torch.manual_seed(0)
    gs = [N.build_generator_module(3 * TG, 3, 3 * (TG - 1), ngf, "composite", 3, "batch", 0, **G_OPT)]
    for s in range(1, n_scales):
        gs.append(N.build_generator_module(3 * TG, 3, 3 * (TG - 1), ngf // 2 ** s, "composite-local", 3, "batch", s, **G_OPT))
    for g in gs:
        g.to(dev).train()
        g.compute_dtype = torch.bfloat16
    return gs


def literal_frames(netG, frames_u8, n_scales):
    """(a): uint8 device frames in, uint8 host images out, with nothing from ir2rgb_amd.inference."""
    from ir2rgb_amd.vid2vid import avg_pool_pyramid
    A_all = torch.stack([f.permute(2, 0, 1).float().div(255).sub(0.5).div(0.5) for f in frames_u8]).unsqueeze(0)
    fake_B_prev, out = None, []
    with torch.no_grad():
        for t in range(A_all.shape[1] - TG + 1):
            real_A = A_all[:, t:t + TG]
            first = fake_B_prev is None
            if first:
                fake_B_prev = [B[0] for B in avg_pool_pyramid(torch.zeros_like(real_A[:, :TG - 1]), n_scales)]
            real_A = avg_pool_pyramid(real_A.contiguous(), n_scales)
            feat = flow_feat = None
            for s in range(n_scales):
                si = n_scales - 1 - s
                h, w = real_A[si].shape[-2:]
                o = netG[s](real_A[si][0, :TG].reshape(1, -1, h, w), fake_B_prev[si].reshape(1, -1, h, w), None, feat, flow_feat,
                            None, first)
                fake_B, feat, flow_feat = o[0], o[4], o[5]
                fake_B_prev[si] = torch.cat([fake_B_prev[si][1:], fake_B])
            image_numpy = fake_B[0].cpu().float().numpy()                  # util.tensor2im (util/util.py:59-68)
            image_numpy = np.clip((np.transpose(image_numpy, (1, 2, 0)) + 1) / 2.0 * 255.0, 0, 255)
            out.append(image_numpy.astype(np.uint8))
    return out


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    n = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def kernel_times(dev, H, W, reps=200):
    from ir2rgb_amd import inference as I, metrics as M
    frame = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device=dev)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    h0, h1 = torch.zeros(TG, 3, H, W, device=dev), torch.zeros(TG, 3, Ho, Wo, device=dev)
    truth = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device=dev)
    x, hb, img = torch.rand(3, H, W, device=dev) * 2 - 1, torch.zeros(TG - 1, 3, H, W, device=dev), torch.zeros(H, W, 3, dtype=torch.uint8, device=dev)

    def many(f):
        def run():
            for _ in range(reps):
                f()
            return reps
        run()
        return timed(run) * 1e3     # us per launch

    px, pp = 3 * H * W, 3 * Ho * Wo
    res = {}
    for name, f, byts in (
            ("frame_push_u8 (T=3, two levels)", lambda: I.frame_push(frame, h0, h1), px + (2 * TG - 1) * 4 * (px + pp)),
            ("frame_push_u8 (T=3, one level)", lambda: I.frame_push(frame, h0), px + (2 * TG - 1) * 4 * px),
            ("frame_finish_u8 (T=2, uint8 image)", lambda: I.frame_finish(x, hb, img), 4 * px + (2 * (TG - 1) - 1) * 4 * px + px),
            # both uint8 frames are read by the reduce pass and again (from L2 / Infinity Cache) by the window pass
            ("video_metrics_u8 (one frame, three launches)", lambda: M.video_metrics(truth, frame), 2 * 2 * px),
            # both uint8 frames once (and six fp64 cube roots per pixel, which no byte count shows)
            ("colour_metrics_u8 (one frame, two launches)", lambda: M.colour_metrics(truth, frame), 2 * px)):
        us = many(f)
        res[name] = {"us_per_launch": round(us, 2), "bytes_moved": int(byts), "GB_per_s": round(byts / us / 1e3, 1)}
    res.update(scale_times(dev, many))
    res.update(agc_times(dev, many))
    res["note"] = ("bytes_moved counts the in-place history shift (slots read and written) beside the frame itself: "
                   f"{px / 1e6:.2f} MB of bytes and {4 * px / 1e6:.2f} MB of fp32 per full-size frame")
    return res


def agc_times(dev, many, hs=512, ws=640, C=3):
    """ThermalAGC (three launches per call) on one raw frame of the camera's size, a narrow-band scene: the histogram and
    the map pass read the 16-bit frame once each, the table pass reads and zeroes the 256 KB of bins, reads and writes the
    512 KB of state twice over and writes the 64 KB table; the map pass writes the uint8 frame."""
    from ir2rgb_amd.thermal import ThermalAGC
    g = torch.Generator().manual_seed(0)
    raw = (7000 + 40 * torch.randn(hs, ws, generator=g)).round().clamp(0, 65535).to(torch.int16).to(dev)
    agc = ThermalAGC(dev, hs, ws, channels=C)
    out = agc(raw)
    us = many(lambda: agc(raw, out=out))
    byts = 2 * 2 * hs * ws + 2 * 4 * 65536 + 3 * 8 * 65536 + 65536 + hs * ws * C
    return {f"thermal_agc_u16 {hs}x{ws} -> uint8 x{C} (one frame, three launches)": {
        "us_per_call": round(us, 2), "bytes_moved": int(byts), "GB_per_s": round(byts / us / 1e3, 1)}}


def scale_times(dev, many, hs=512, ws=640, C=3):
    """FrameScaler (two launches per call) at the camera size of the KAIST frames: per target size and output form one row
    with the bytes each pass moves, computed from the shapes -- the horizontal pass reads the source rows the kept output
    rows need and writes them scaled into the workspace, the vertical pass reads the workspace once (the overlapping taps
    of neighbouring output rows are re-reads of lines just fetched) and writes the result.  The entry point is called
    directly (no Python wrapper in the timed loop).  It enqueues both launches, so ``us_per_call`` and ``GB_per_s`` are
    figures of the pair; the time of each pass comes from a kernel trace of ``--kernels-only`` (scale_h_kernel /
    scale_v_kernel rows), to be set against ``horizontal_pass_bytes`` / ``vertical_pass_bytes``."""
    from ir2rgb_amd import _lib
    from ir2rgb_amd.transform import FrameScaler
    src = torch.randint(0, 256, (hs, ws, C), dtype=torch.uint8, device=dev)
    res = {}
    for H, W in ((832, 1024), (416, 512)):
        sc = FrameScaler(dev, (hs, ws), C, (W, H))
        rows = sc.workspace_bytes(1) // (W * C)
        for normalised in (False, True):
            out = sc(src, normalised=normalised)
            h_bytes = rows * ws * C + rows * W * C
            v_bytes = rows * W * C + H * W * C * (4 if normalised else 1)
            (xb, xc, xk), (yb, yc, yk) = sc.x_tables, sc.y_tables
            args = (src, out, sc._ws, sc.workspace_bytes(1), xb, xc, xk, yb, yc, yk, 1, *sc._geom, int(sc.flip), int(normalised),
                    _lib.current_stream(src))
            entry = _lib.lib().ir2rgb_frame_scale_u8
            us = many(lambda: entry(*args))
            res[f"frame_scale_u8 {hs}x{ws}x{C} -> {H}x{W} ({'fp32 planar' if normalised else 'uint8'}, two launches)"] = {
                "us_per_call": round(us, 2), "horizontal_pass_bytes": int(h_bytes), "vertical_pass_bytes": int(v_bytes),
                "bytes_moved": int(h_bytes + v_bytes), "GB_per_s": round((h_bytes + v_bytes) / us / 1e3, 1)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels-only", action="store_true",
                    help="only the frame-I/O, score and scaling kernels (short: the run to put under a kernel trace)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_infer.py needs the GPU (there is nothing to measure without one)")
    from ir2rgb_amd.inference import VideoTranslator
    dev = torch.device("cuda:0")
    H, W = a.height, a.width
    gen = torch.Generator().manual_seed(0)
    frames = list(torch.randint(0, 256, (a.frames + TG - 1, H, W, 3), generator=gen, dtype=torch.uint8).to(dev))
    doc = {"device": torch.cuda.get_device_name(0), "height": H, "width": W, "dtype": "bf16", "frames": a.frames,
           "warmup_frames": a.warmup, "rounds": a.rounds, "configs": {}}
    try:
        doc["commit"] = subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, text=True,
                                                stderr=subprocess.DEVNULL).strip()
    except Exception:  # noqa: BLE001  (a snapshot without history)
        doc["commit"] = None
    for name, ns in (() if a.kernels_only else (("one scale, ngf 128", 1), ("two scales, ngf 128 / 64", 2))):
        netG = build(ns, 128, dev)
        kw = dict(netG=netG, n_scales_spatial=ns, first_layer_gen_filters=128, first_frame="zeros", compute_dtype=torch.bfloat16)
        tr = {"eager": VideoTranslator(dev, H, W, use_graph=False, **kw), "graph": VideoTranslator(dev, H, W, use_graph=True, **kw)}
        ways = {"literal": lambda: len(literal_frames(netG, frames, ns)),
                "eager": lambda: len(list(tr["eager"].translate(frames))),
                "graph": lambda: len(list(tr["graph"].translate(frames)))}
        warm = frames[:a.warmup + TG - 1]
        literal_frames(netG, warm, ns)
        for t in tr.values():
            list(t.translate(warm))
        ms = {k: [] for k in ways}
        for _ in range(a.rounds):
            for k, f in ways.items():
                ms[k].append(timed(f))
        doc["configs"][name] = {k: {"ms_per_frame": round(statistics.median(v), 3),
                                    "frames_per_s": round(1e3 / statistics.median(v), 2),
                                    "rounds_ms": [round(x, 3) for x in v]} for k, v in ms.items()}
        del tr, netG
        torch.cuda.empty_cache()
    doc["frame_kernels"] = kernel_times(dev, H, W)
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
