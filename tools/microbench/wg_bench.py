"""Times of the weight-gradient family (csrc/wgrad_mfma.hip: kernel + finish pass) at each form the 512x1024 training window
launches (shapes of tests/window_geometries.json), one line per shape:  <name> <microseconds per call>.  One process = one
sample; compare two builds by alternating processes.

    python tools/microbench/wg_bench.py [substring of the names to run]

nine     conv_wgrad3x3_kernel (3x3 stride 1, reflection): the bottleneck blocks and the 128-channel blocks of the finest scale
line     conv_wgrad_line_kernel: the stride-2 3x3 down- / up-samplers at both ends of the channel range, the 1x7 head
col      conv_wgrad_col_kernel: 7x1 at stride 1, the discriminators' 4x1 at stride 2
onetap   conv_wgrad_kernel: tap pairs (Cin = 64), one tap per workgroup, and the accumulating call of a shared parameter
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

from ir2rgb_amd import conv as C  # noqa: E402

dev = torch.device("cuda:0")
dt = torch.bfloat16
only = sys.argv[1] if len(sys.argv) > 1 else ""


def nhwc(*shape):
    return torch.randn(*shape, device=dev).to(dt).contiguous(memory_format=torch.channels_last)


def timed(name, fn, calls=50):
    if only not in name:
        return
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    e.record()
    torch.cuda.synchronize()
    print(name, "%.2f" % (a.elapsed_time(e) * 1000 / calls), flush=True)


# (name, N, Cin, H, W, Cout, kernel, stride, pad, pad_mode, transposed, accumulate)
SHAPES = (
    ("nine/1024-1024@32x64", 1, 1024, 32, 64, 1024, 3, 1, 1, 1, False, False),
    ("nine/128-128@256x512", 1, 128, 256, 512, 128, 3, 1, 1, 1, False, False),
    ("line/3x3s2/64-128@512x1024", 1, 64, 512, 1024, 128, 3, 2, 1, 0, False, False),
    ("line/3x3s2/512-1024@64x128", 1, 512, 64, 128, 1024, 3, 2, 1, 0, False, False),
    ("line/3x3s2T/1024-512@32x64", 1, 1024, 32, 64, 512, 3, 2, 1, 0, True, False),
    ("line/3x3s2T/128-64@256x512", 1, 128, 256, 512, 64, 3, 2, 1, 0, True, False),
    ("col/7x1/64-64@512x1024", 1, 64, 512, 1024, 64, (7, 1), 1, (3, 0), 1, False, False),
    ("col/7x1/64-128@256x512", 1, 64, 256, 512, 128, (7, 1), 1, (3, 0), 1, False, False),
    ("col/4x1s2/n3/64-64@512x513", 3, 64, 512, 513, 64, (4, 1), (2, 1), (2, 0), 0, False, False),
    ("line/1x7/64-64@512x1024", 1, 64, 512, 1024, 64, (1, 7), 1, (0, 3), 1, False, False),
    ("onetap/4x4s2/n3/64-128@257x513", 3, 64, 257, 513, 128, 4, 2, 2, 0, False, False),
    ("onetap/3x3s2/128-256@256x512", 1, 128, 256, 512, 256, 3, 2, 1, 0, False, False),
    ("onetap/acc/4x4s1/n3/512-8@66x130", 3, 512, 66, 130, 8, 4, 1, 2, 0, False, True),
)

for name, n, cin, h, w, cout, k, s, p, pm, tr, acc in SHAPES:
    if only not in name:
        continue
    x = nhwc(n, cin, h, w)
    d = C.make_desc(tuple(x.shape), cout, k, s, p, pm, dt, tr, 1 if tr else 0)
    gy = nhwc(n, cout, d.Hout, d.Wout)
    if acc:
        out = torch.zeros(C.conv2d_wgrad(d, x, gy).shape, device=dev)
        timed(name, lambda: C.conv2d_wgrad(d, x, gy, out=out, accumulate=True))
    else:
        timed(name, lambda: C.conv2d_wgrad(d, x, gy))
    del x, gy
