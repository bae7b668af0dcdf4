"""Times of the HBM-bound BatchNorm / pointwise family (csrc/pointwise.hip, backward.hip) at the workload's shapes, one line
per shape:  <name> <microseconds per call>.  One process = one sample; compare two builds by alternating processes.

    python tools/microbench/bn_family_bench.py [substring of the names to run]

bn_bwd        one-pass (few pixels per channel), reduce + fused finalize/apply (512x1024 layers), activation-only
bn_finalize   statistics alone, both block shapes (rows >= 2048 and C <= 256: 8 channels per block)
bn_fused      statistics + apply in one launch (the residual blocks), bn_apply: the plain apply
xexpand_bwd   the tile kernel, and the per-pixel kernel (a 2-byte misaligned gradient sends the call there)
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

from ir2rgb_amd import _lib  # noqa: E402
from ir2rgb_amd import autograd as A  # noqa: E402
from ir2rgb_amd import layers as L  # noqa: E402

dev = torch.device("cuda:0")
only = sys.argv[1] if len(sys.argv) > 1 else ""


def nhwc(C, H, W):
    return torch.randn(1, C, H, W, device=dev).bfloat16().contiguous(memory_format=torch.channels_last)


def timed(name, fn, calls=100):
    if only not in name:
        return
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    e.record()
    torch.cuda.synchronize()
    print(name, "%.2f" % (a.elapsed_time(e) * 1000 / calls), flush=True)


# one-pass: 1024 x 32x64 (K = 4), 512 x 33x65 (K = 8), 2048 channels (16 per block); two launches: 64-128 x 512x1024
for C, H, W in ((1024, 32, 64), (512, 33, 65), (2048, 16, 32), (2048, 32, 64), (64, 512, 1024), (128, 512, 1024)):
    y, gz = nhwc(C, H, W), nhwc(C, H, W)
    v = [torch.rand(C, device=dev) + 0.5 for _ in range(4)]
    out = torch.empty_like(y)
    timed(f"bn_bwd/{C}x{H}x{W}", lambda: A.bn_bwd(gz, y, v[0], v[1], v[2], v[3], 1, out=out))
    if C <= 128:
        timed(f"bn_bwd/act_only/{C}x{H}x{W}", lambda: A.bn_bwd(gz, y, None, None, None, None, 2, out=out))

for rows, ch in ((16384, 64), (4096, 64), (4096, 128), (2048, 512), (64, 1024)):
    stats = torch.rand(rows, 2, ch, device=dev)
    bn = torch.nn.BatchNorm2d(ch).to(dev)
    timed(f"bn_finalize/{rows}x{ch}", lambda: L.bn_finalize(stats, rows * 128, bn, True, None))

for C, H, W, rows, res in ((1024, 32, 64, 16, 1), (1024, 32, 64, 16, 0), (512, 64, 128, 64, 0), (256, 64, 128, 128, 1)):
    y, z = nhwc(C, H, W), nhwc(C, H, W)
    r1 = nhwc(C, H, W) if res else None
    stats = torch.rand(rows, 2, C, device=dev)
    bn = torch.nn.BatchNorm2d(C).to(dev)
    timed(f"bn_fused/{C}x{H}x{W}/rows{rows}/res{res}", lambda: L.bn_finalize_apply(stats, H * W, bn, y, 1, res1=r1, out=z))
    sc, sh = torch.rand(C, device=dev) + 0.5, torch.rand(C, device=dev)
    timed(f"bn_apply/{C}x{H}x{W}/res{res}", lambda: L.bn_apply(y, sc, sh, 1, res1=r1, out=z))
y, z = nhwc(64, 512, 1024), nhwc(64, 512, 1024)
sc, sh = torch.rand(64, device=dev) + 0.5, torch.rand(64, device=dev)
timed("bn_apply/64x512x1024/res0", lambda: L.bn_apply(y, sc, sh, 1, out=z))

for cin, H, W, kw, sx, px, pm in ((6, 512, 1024, 4, 2, 2, 0), (15, 512, 1024, 4, 2, 2, 0), (6, 256, 512, 4, 2, 2, 0), (9, 512, 1024, 7, 1, 3, 1)):
    wout = (W + 2 * px - kw) // sx + 1
    d = nhwc(64, H, wout)
    timed(f"xexpand_bwd/tile/{cin}x{H}x{W}k{kw}s{sx}", lambda: A.xexpand_bwd(d, cin, W, kw, sx, px, pm))
    flat = torch.randn(H * wout * 64 + 8, device=dev).bfloat16()
    din = torch.empty(1, cin, H, W, device=dev)
    timed(f"xexpand_bwd/pixel/{cin}x{H}x{W}k{kw}s{sx}",
          lambda: _lib.lib().ir2rgb_xexpand_bwd(flat[1:], din, 1, cin, H, W, wout, kw, sx, px, pm, 1, _lib.current_stream(din)), calls=30)
