"""ir2rgb_ema_step beside ir2rgb_adam_step over the full-size generators' parameter table, in one process:

    python tools/microbench/ema_bench.py [--scales 2] [--calls 100] [--samples 5]

Both kernels stream the same tensors through the same (tensor, chunk) block map; Adam moves 28 bytes per parameter, the
average 12.  A sample is ``--calls`` back-to-back launches between two device events; the two kernels' samples alternate.
Adam's bytes per second in this run is the yardstick for the average's, and the spread of Adam's samples the margin."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

from ir2rgb_amd import _lib  # noqa: E402
from ir2rgb_amd import optim as OP  # noqa: E402
from ir2rgb_amd import vid2vid as V  # noqa: E402
from ir2rgb_amd.inference import VideoTranslator  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scales", type=int, default=2)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--samples", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "ema_bench needs the GPU"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    gens = VideoTranslator._build_generators(dict(V.DEFAULTS, n_scales_spatial=a.scales))
    params = [p for g in gens for p in g.to(dev).parameters()]
    n = sum(p.numel() for p in params)
    for p in params:
        p.grad = torch.randn_like(p) * 0.01
    adam = OP.FusedAdam(params, lr=2e-4, betas=(0.5, 0.999))
    ema = OP.ParamEMA(params, 0.999)
    adam._refresh_table()
    nb_a, nb_e = adam._blocks.shape[0], ema._blocks.shape[0]
    assert nb_a == nb_e
    step = [0]

    def adam_call():
        step[0] += 1
        _lib.launch("ir2rgb_adam_step", adam.exp_avg, adam._rows_dev, adam._blocks, nb_a, 2e-4, 0.5, 0.999, 1e-8, step[0])

    def ema_call():
        _lib.launch("ir2rgb_ema_step", ema.buf, ema._rows_dev, ema._blocks, nb_e, ema.state, None, ema.beta, 1)

    def sample(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.calls * 1e3      # us per call

    for fn in (adam_call, ema_call):
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    us = {"adam": [], "ema": []}
    for _ in range(a.samples):
        us["adam"].append(sample(adam_call))
        us["ema"].append(sample(ema_call))
    print(f"{len(params)} tensors, {n / 1e6:.1f} M parameters, {nb_a} blocks; {a.calls} calls per sample, {a.samples} samples each")
    for name, nbytes in (("adam", 28), ("ema", 12)):
        t = us[name]
        gbs = [n * nbytes / x / 1e3 for x in t]
        print(f"{name:5s} {nbytes} B/param  us per call: " + " ".join(f"{x:.1f}" for x in t) +
              f"  median {statistics.median(t):.1f} (min {min(t):.1f} max {max(t):.1f})")
        print(f"{name:5s} GB/s: " + " ".join(f"{x:.0f}" for x in gbs) +
              f"  median {statistics.median(gbs):.0f} (min {min(gbs):.0f} max {max(gbs):.0f})")
    st = ema.stats()
    assert st["updates"] == 10 + a.calls * a.samples and bool(torch.isfinite(ema.buf).all())


if __name__ == "__main__":
    main()
