"""ir2rgb_visuals_u8 on the nine panels of a training snapshot, beside the reference's way of making them, in one process:

    python tools/microbench/visuals_bench.py [--height 512] [--width 1024] [--calls 100] [--samples 5]

The call reads 21 fp32 planes for the panels and 4 of them once more for the two flow ranges, and writes 3 bytes per
pixel and panel: 58 MB + 8 MB at 512x1024.  A sample is ``--calls`` back-to-back calls between two device events; the
bytes per second are stated against the 58 MB of the panels themselves (44 MB read, 14 MB written).  Two figures: the
same buffers every call (58 MB stay in the 256 MB Infinity Cache: the warm figure, what a snapshot right after the window
that wrote its sources sees at best), and ``--sets`` copies of sources and stack taken in turn (10 x 58 MB: every call's
data was last touched ten calls ago and comes from HBM).  The comparison is the
same nine conversions done as util.save_all_tensors does them: each tensor ``.cpu()``, converted in numpy (wall time per
snapshot, the forced synchronisation included; the flow panels through ``flow_to_rgb_reference``, OpenCV being absent)."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

from ir2rgb_amd import visuals as V  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--host-samples", type=int, default=3)
    ap.add_argument("--sets", type=int, default=10)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "visuals_bench needs the GPU"
    dev = torch.device("cuda:0")
    h, w = a.height, a.width
    g = torch.Generator().manual_seed(0)
    r = lambda *s: (torch.randn(s, generator=g) * 0.8).to(dev)  # noqa: E731
    t = dict(real_A=r(1, 1, 3, h, w), fake_B=r(1, 1, 3, h, w), fake_B_first=r(3, h, w), fake_B_raw=r(1, 1, 3, h, w),
             real_B=r(1, 1, 3, h, w), flow_ref=r(1, 1, 2, h, w) * 4, conf_ref=torch.rand((1, 1, 1, h, w), generator=g).to(dev),
             flow=r(1, 1, 2, h, w) * 4, weight=torch.rand((1, 1, 1, h, w), generator=g).to(dev))
    plist = V.panels(t, {"input_nc": 3})
    planes = sum(x.shape[0] for _, _, x in plist)
    assert len(plist) == 9 and planes == 21
    out = torch.empty((9, h, w, 3), dtype=torch.uint8, device=dev)
    ws = torch.empty(V.workspace_elems(2, h, w), dtype=torch.float32, device=dev)
    moved = planes * h * w * 4 + out.numel()

    sets = [(plist, out)] + [([(n, k, x.clone()) for n, k, x in plist], torch.empty_like(out)) for _ in range(a.sets - 1)]

    def sample(n_sets):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(a.calls):
            pl, o = sets[i % n_sets]
            V.compose(pl, o, ws)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.calls * 1e3      # us per call

    print(f"nine panels at {h}x{w}: {planes} fp32 planes, {moved / 1e6:.1f} MB moved; {a.calls} calls per sample, {a.samples} samples")
    for label, n_sets in (("same buffers", 1), (f"{a.sets} buffer sets in turn", a.sets)):
        for i in range(10):
            V.compose(*sets[i % n_sets], ws)
        torch.cuda.synchronize()
        us = [sample(n_sets) for _ in range(a.samples)]
        gbs = [moved / x / 1e3 for x in us]
        print(f"device, {label}  us per call: " + " ".join(f"{x:.1f}" for x in us) +
              f"  median {statistics.median(us):.1f} (min {min(us):.1f} max {max(us):.1f})")
        print(f"device, {label}  GB/s: " + " ".join(f"{x:.0f}" for x in gbs) + f"  median {statistics.median(gbs):.0f}")
    host = []
    for _ in range(a.host_samples):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        V.reference_images(plist)
        host.append((time.perf_counter() - t0) * 1e3)
    print("host (.cpu() + numpy)  ms per snapshot: " + " ".join(f"{x:.0f}" for x in host) + f"  median {statistics.median(host):.0f}")


if __name__ == "__main__":
    main()
