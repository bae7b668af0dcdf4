"""ir2rgb_thermal_agc_u16 on one raw frame, beside the same definition in eager torch on the device, in one process:

    python tools/microbench/agc_bench.py [--height 512] [--width 640] [--calls 100] [--samples 5] [--out FILE]

Two scenes: a narrow band (a smooth background near 7000 counts, a warmer block, sensor noise of a few counts: some
hundreds of occupied levels, what a microbolometer delivers) and the full range (uniform random over all 65536 levels: no
two neighbours equal, no contention either).  A sample is ``--calls`` back-to-back calls on the same frame between two
device events, after ten warm-up calls; the state keeps advancing, as it does on a camera.  The comparison is the
definition statement by statement in eager torch on the device -- ``bincount``, ``clamp``, the Q16 blend in int64,
``cumsum``, the table, a gather -- which synchronises with the host once per frame where ``bincount`` sizes its result.
Both are checked against each other on the frame before anything is timed.  Prints the lines it measures and, with
``--out``, writes them to that file too."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

from ir2rgb_amd.thermal import LEVELS, ThermalAGC  # noqa: E402


class EagerAGC:
    """The definition of ir2rgb_amd.thermal in eager torch (int64 on the device)."""

    def __init__(self, agc):
        self.mode, self.plateau, self.k, self.tail, self.C = agc._mode, agc.plateau, 65536 - agc.a_q, agc.tail_ppm, agc.channels
        self.S = None
        self.v = torch.arange(LEVELS, device=agc.device)

    def __call__(self, raw_i16):
        x = raw_i16.long() & 0xffff
        h = torch.bincount(x.reshape(-1), minlength=LEVELS)
        G = (h.clamp(max=self.plateau) if self.mode == 0 else h) << 16
        self.S = G if self.S is None else self.S + (((G - self.S) * self.k) >> 16)
        C = torch.cumsum(self.S, 0)
        T = C[-1]
        if self.mode == 0:
            c0 = C[torch.argmax((self.S > 0).to(torch.uint8))]
            D = T - c0
            lut = torch.div((C - c0).clamp(min=0) * 255 + torch.div(D, 2, rounding_mode="floor"), D.clamp(min=1), rounding_mode="floor")
            lut = torch.where(D > 0, lut, torch.zeros_like(lut))
        else:
            lo = torch.argmax((C * 1000000 > T * self.tail).to(torch.uint8))
            hi = torch.argmax((C * 1000000 >= T * (1000000 - self.tail)).to(torch.uint8))
            Wd = hi - lo
            lut = torch.div((self.v - lo) * 255 + torch.div(Wd, 2, rounding_mode="floor"), Wd.clamp(min=1), rounding_mode="floor")
            lut = torch.where(Wd > 0, lut.clamp(0, 255), torch.zeros_like(lut))
        return lut.to(torch.uint8)[x].unsqueeze(-1).expand(-1, -1, self.C).contiguous()


def scenes(h, w, g):
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    f = 7000 + 300 * torch.sin(xx / 90.0) * torch.cos(yy / 70.0) + 6 * torch.randn(h, w, generator=g)
    f[h // 4:h // 2, w // 3:w // 2] += 2500
    narrow = f.round().clamp(0, 65535).to(torch.int32)
    full = torch.randint(0, 65536, (h, w), generator=g, dtype=torch.int32)
    return {"narrow band": narrow, "full range": full}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "agc_bench needs the GPU"
    dev = torch.device("cuda:0")
    h, w = a.height, a.width
    g = torch.Generator().manual_seed(0)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def sample(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.calls * 1e3      # us per call

    say(f"one raw frame at {h}x{w}: {a.calls} calls per sample after 10 warm-up calls, {a.samples} samples")
    for name, counts in scenes(h, w, g).items():
        raw = counts.to(torch.int16).to(dev)            # the low 16 bits: the camera's counts
        occupied = int(torch.unique(counts).numel())
        for mode in ("plateau", "linear"):
            agc = ThermalAGC(dev, h, w, mode=mode, channels=3)
            eager = EagerAGC(agc)
            out = torch.empty((h, w, 3), dtype=torch.uint8, device=dev)
            same = all(torch.equal(agc(raw, out=out), eager(raw)) for _ in range(3))
            assert same and torch.equal(agc.state(), eager.S), f"{name} {mode}: the kernels and eager torch disagree"
            for what, fn in (("ir2rgb_thermal_agc_u16", lambda: agc(raw, out=out)), ("eager torch int64", lambda: eager(raw))):
                for _ in range(10):
                    fn()
                torch.cuda.synchronize()
                us = [sample(fn) for _ in range(a.samples)]
                say(f"{name} ({occupied} levels), {mode}, {what}  us per call: " + " ".join(f"{x:.1f}" for x in us) +
                    f"  median {statistics.median(us):.1f} (min {min(us):.1f} max {max(us):.1f})")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
