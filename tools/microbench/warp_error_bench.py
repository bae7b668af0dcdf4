"""ir2rgb_warp_error_u8 on one pair of frames, beside the same quantity the way the trainer forms it, in one process:

    python tools/microbench/warp_error_bench.py [--height 512] [--width 1024] [--calls 100] [--samples 5]

The call reads both uint8 frames (prev gathered, cur streamed: 3.1 MB at 512x1024), the flow (4.2 MB) and the weight
(2.1 MB) and writes three doubles.  A sample is ``--calls`` back-to-back calls between two device events.  Two figures: the
same buffers every call (9.4 MB stay in the 256 MB Infinity Cache: the warm figure, what a score right after the step that
wrote the frame sees at best), and ``--sets`` copies of all four inputs taken in turn (40 x 9.4 MB: every call's data was
last touched forty calls ago and comes from HBM).  The comparison is ``vid2vid.masked_l1(cur, vid2vid.resample(prev, flow),
conf)`` on the normalised fp32 frames (eager torch: the lattice, grid_sample, two products, l1_loss), which is warp_l1 alone,
in fp32, and leaves the 8-bit frames still to be normalised."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

from ir2rgb_amd import metrics, vid2vid as V  # noqa: E402
from ir2rgb_amd.inference import normalise_u8  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--sets", type=int, default=40)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "warp_error_bench needs the GPU"
    dev = torch.device("cuda:0")
    h, w = a.height, a.width
    g = torch.Generator().manual_seed(0)

    def one_set():
        return (torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8).to(dev),
                torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8).to(dev),
                (torch.randn((2, h, w), generator=g) * 3).to(dev), (torch.rand((1, h, w), generator=g) < 0.7).float().to(dev))

    sets = [one_set() for _ in range(a.sets)]
    moved = sum(t.numel() * t.element_size() for t in sets[0])
    torch_sets = [(normalise_u8(p).unsqueeze(0).contiguous(), normalise_u8(c).unsqueeze(0).contiguous(), f.unsqueeze(0),
                   m.unsqueeze(0)) for p, c, f, m in sets]

    def kernel(i, n_sets):
        return metrics.warp_error(*sets[i % n_sets])

    def eager(i, n_sets):
        p, c, f, m = torch_sets[i % n_sets]
        return V.masked_l1(c, V.resample(p, f), m)

    def sample(fn, n_sets):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(a.calls):
            fn(i, n_sets)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.calls * 1e3      # us per call

    got, want = float(kernel(0, 1)[0, 0]), float(eager(0, 1))
    print(f"one pair at {h}x{w}: {moved / 1e6:.1f} MB read; {a.calls} calls per sample, {a.samples} samples; "
          f"warp_l1 {got:.9f} (kernel, fp64) {want:.9f} (resample + masked_l1, fp32)")
    for what, fn in (("ir2rgb_warp_error_u8", kernel), ("resample + masked_l1", eager)):
        for label, n_sets in (("same buffers", 1), (f"{a.sets} buffer sets in turn", a.sets)):
            for i in range(10):
                fn(i, n_sets)
            torch.cuda.synchronize()
            us = [sample(fn, n_sets) for _ in range(a.samples)]
            print(f"{what}, {label}  us per call: " + " ".join(f"{x:.1f}" for x in us) +
                  f"  median {statistics.median(us):.1f} (min {min(us):.1f} max {max(us):.1f})")
            if fn is kernel:
                gbs = [moved / x / 1e3 for x in us]
                print(f"{what}, {label}  GB/s: " + " ".join(f"{x:.0f}" for x in gbs) + f"  median {statistics.median(gbs):.0f}")


if __name__ == "__main__":
    main()
