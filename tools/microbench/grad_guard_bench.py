"""The checked optimizer step, with a guard and with a loss scaler, beside the plain one over the full-size generators'
parameter table, in one process:

    python tools/microbench/grad_guard_bench.py [--scales 2] [--calls 100] [--samples 5]

    guard     ir2rgb_grad_check + ir2rgb_adam_step_checked   (check, finish, step: 32 bytes per parameter; every step clipped)
    plain     ir2rgb_adam_step                               (28 bytes per parameter)
    scaler    ir2rgb_grad_check + ir2rgb_adam_step_checked   (the same kernels: no guard block, max_norm inf)

A sample is ``--calls`` back-to-back steps between two device events; the variants' samples alternate.  The plain step's
bytes per second in this run is the yardstick, and the spread of its samples (max - min) the margin within which the
two checked medians are expected to agree."""
import argparse
import math
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
    assert torch.cuda.is_available(), "grad_guard_bench needs the GPU"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    gens = VideoTranslator._build_generators(dict(V.DEFAULTS, n_scales_spatial=a.scales))
    params = [p for g in gens for p in g.to(dev).parameters()]
    n = sum(p.numel() for p in params)
    for p in params:
        p.grad = torch.randn_like(p) * 0.01
    adam = OP.FusedAdam(params, lr=2e-4, betas=(0.5, 0.999))
    guard = OP.GradGuard(adam, 1.0)                    # (the gradient's norm is ~190: every step is clipped)
    scaler = OP.LossScaler(dev, init_scale=1.0, growth_interval=0)
    adam._refresh_table()
    state, nb = adam.scaled_state(), adam._blocks.shape[0]
    step = [0]

    def plain_call():
        step[0] += 1
        _lib.launch("ir2rgb_adam_step", adam.exp_avg, adam._rows_dev, adam._blocks, nb, 2e-4, 0.5, 0.999, 1e-8, step[0])

    def checked_call(guard_state, scaler_state, max_norm):
        _lib.launch("ir2rgb_grad_check", adam.exp_avg, adam._rows_dev, adam._blocks, nb, adam._partial, state, guard_state,
                    scaler_state, max_norm, 2e-4, 0.5, 0.999, 1e-8)
        _lib.launch("ir2rgb_adam_step_checked", adam.exp_avg, adam._rows_dev, adam._blocks, nb, state)

    def scaler_call():
        checked_call(None, scaler.state, math.inf)

    def guard_call():
        checked_call(guard.state, None, guard.max_norm)

    def sample(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.calls * 1e3      # us per call

    variants = (("guard", guard_call, 32), ("plain", plain_call, 28), ("scaler", scaler_call, 32))
    for _, fn, _ in variants:
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    us = {name: [] for name, _, _ in variants}
    for _ in range(a.samples):
        for name, fn, _ in variants:
            us[name].append(sample(fn))
    print(f"{len(params)} tensors, {n / 1e6:.1f} M parameters, {nb} blocks; {a.calls} calls per sample, {a.samples} samples each")
    for name, _, nbytes in variants:
        t = us[name]
        tbs = [n * nbytes / x / 1e6 for x in t]
        print(f"{name:8s} {nbytes} B/param  us per call: " + " ".join(f"{x:.1f}" for x in t) +
              f"  median {statistics.median(t):.1f} (min {min(t):.1f} max {max(t):.1f})")
        print(f"{name:8s} TB/s: " + " ".join(f"{x:.2f}" for x in tbs) +
              f"  median {statistics.median(tbs):.2f} (min {min(tbs):.2f} max {max(tbs):.2f})")
    spread = max(us["plain"]) - min(us["plain"])
    diff = statistics.median(us["guard"]) - statistics.median(us["scaler"])
    print(f"guard / plain medians: {statistics.median(us['guard']) / statistics.median(us['plain']):.3f} (32 / 28 = 1.143 by bytes)")
    print(f"guard - scaler medians: {diff:+.1f} us; the plain step's max - min spread: {spread:.1f} us")
    st = guard.stats()
    assert st["steps"] == 10 + a.calls * a.samples and st["skipped"] == 0 and st["clipped"] == st["steps"], st
    assert all(bool(torch.isfinite(p).all()) for p in params[:4])


if __name__ == "__main__":
    main()
