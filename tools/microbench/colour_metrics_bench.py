"""ir2rgb_colour_metrics_u8 on one pair of frames, beside the same definition in eager torch on the device, in one process:

    python tools/microbench/colour_metrics_bench.py [--height 512] [--width 1024] [--calls 100] [--samples 5] [--out FILE]

The call reads both uint8 frames (3.1 MB at 512x1024) and the 2 KB table and writes five doubles; per pixel it does about a
hundred fp64 operations and six cube roots (counted from the formula: 0.1 GFLOP a frame without the roots).  A sample is
``--calls`` back-to-back calls between two device events.  Two figures: the same buffers every call (3.1 MB stay in the
256 MB Infinity Cache: the warm figure, what a score right after the step that wrote the frame sees at best), and ``--sets``
copies of both frames taken in turn (100 x 3.1 MB: every call's data was last touched a hundred calls ago and comes from
HBM).  The comparison is the module's definition statement by statement in eager torch fp64 on the device -- the table
lookup, the three rows, ``torch.pow(t, 1/3)`` for the cube root (torch has no cbrt), the five means -- some sixty launches
over [H,W] fp64 temporaries.  Prints the lines it measures and, with ``--out``, writes them to that file too."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

from ir2rgb_amd import metrics  # noqa: E402


def eager_rows(orig, pred, lin):
    """[5] on the device: the definition in eager torch, with pow for the cube root."""
    H, W = orig.shape[:2]

    def lab(img):
        v = lin[img.long()]
        r, g, b = v[..., 0], v[..., 1], v[..., 2]
        tx = (0.412453 * r + 0.357580 * g + 0.180423 * b) / 0.95047
        ty = (0.212671 * r + 0.715160 * g + 0.072169 * b) / 1.0
        tz = (0.019334 * r + 0.119193 * g + 0.950227 * b) / 1.08883
        fx, fy, fz = (torch.where(t > 0.008856, torch.pow(t, 1.0 / 3.0), 7.787 * t + 16.0 / 116.0) for t in (tx, ty, tz))
        return 116.0 * fy - 16.0, 500.0 * (fx - fy), 200.0 * (fy - fz)

    d = orig.to(torch.float64) - pred.to(torch.float64)
    mse = (d * d).sum() / (3 * H * W)
    (Lo, ao, bo), (Lp, ap, bp) = lab(orig), lab(pred)
    dL, da, db = Lo - Lp, ao - ap, bo - bp
    dE, dC = (dL * dL + da * da + db * db).sqrt(), (da * da + db * db).sqrt()
    return torch.stack([mse, 10.0 * torch.log10(mse.new_tensor(65025.0) / mse), dE.sum() / (H * W), dL.abs().sum() / (H * W),
                        dC.sum() / (H * W)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--sets", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "colour_metrics_bench needs the GPU"
    dev = torch.device("cuda:0")
    h, w = a.height, a.width
    g = torch.Generator().manual_seed(0)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def one_set():
        return (torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8).to(dev),
                torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8).to(dev))

    sets = [one_set() for _ in range(a.sets)]
    moved = sum(t.numel() * t.element_size() for t in sets[0])
    lin = metrics.srgb_table(dev)

    def kernel(i, n_sets):
        return metrics.colour_metrics(*sets[i % n_sets])

    def eager(i, n_sets):
        return eager_rows(*sets[i % n_sets], lin)

    def sample(fn, n_sets):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(a.calls):
            fn(i, n_sets)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.calls * 1e3      # us per call

    got, want = kernel(0, 1)[0].tolist(), eager(0, 1).tolist()
    say(f"one pair at {h}x{w}: {moved / 1e6:.1f} MB read; {a.calls} calls per sample, {a.samples} samples")
    say("kernel rows (mse, psnr, delta_e, delta_l, delta_c) " + " ".join(f"{x:.12g}" for x in got))
    say("eager  rows (pow for the cube root)                " + " ".join(f"{x:.12g}" for x in want))
    for what, fn in (("ir2rgb_colour_metrics_u8", kernel), ("eager torch fp64", eager)):
        for label, n_sets in (("same buffers", 1), (f"{a.sets} buffer sets in turn", a.sets)):
            for i in range(10):
                fn(i, n_sets)
            torch.cuda.synchronize()
            us = [sample(fn, n_sets) for _ in range(a.samples)]
            say(f"{what}, {label}  us per call: " + " ".join(f"{x:.1f}" for x in us) +
                f"  median {statistics.median(us):.1f} (min {min(us):.1f} max {max(us):.1f})")
            if fn is kernel:
                gbs = [moved / x / 1e3 for x in us]
                say(f"{what}, {label}  GB/s: " + " ".join(f"{x:.0f}" for x in gbs) + f"  median {statistics.median(gbs):.0f}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
