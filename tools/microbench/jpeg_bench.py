"""JPEG files of translated frames: encoded on the device (ir2rgb_amd.JpegEncoder, csrc/jpeg.hip) beside what the host does
today, in one process:

    python tools/microbench/jpeg_bench.py [--height 512] [--width 1024] [--frames 50] [--samples 5] [--quality 75]

Per sample, ``--frames`` frames (``--sets`` different ones taken in turn: smooth colour with a noisy band, the content of the
full-size golden) go through

  device, launches only   the three launches of ir2rgb_jpeg_encode_u8 between two device events
  device, to bytes        submit(k) / collect(k - 1): launches, the copy of the length, then exactly that many bytes, to
                          ``bytes`` on the host (wall clock, the pipeline VideoTranslator.save runs)
  host                    the raw frame copied to the host, then Image.save(..., "JPEG", quality=...) on one core (wall
                          clock; restart_marker_rows=1, the file the device writes)

and the bytes that cross to the host are printed for both.  The files of the two paths are compared once."""
import argparse
import io
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "tests", "golden"))
import torch  # noqa: E402

from ir2rgb_amd.jpeg import JpegEncoder  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--sets", type=int, default=8)
    ap.add_argument("--quality", type=int, default=75)
    ap.add_argument("--subsampling", default="4:2:0")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "jpeg_bench needs the GPU"
    from PIL import Image
    from make_jpeg_goldens import fullsize_frame
    dev = torch.device("cuda:0")
    h, w = a.height, a.width
    frames = [torch.from_numpy(fullsize_frame(seed, (h, w))).roll(37 * seed, 1).contiguous().to(dev) for seed in range(a.sets)]
    enc = JpegEncoder(dev, h, w, quality=a.quality, subsampling=a.subsampling)
    pinned = torch.empty((h, w, 3), dtype=torch.uint8, pin_memory=True)

    def host_file(f):
        pinned.copy_(f)
        b = io.BytesIO()
        Image.fromarray(pinned.numpy(), "RGB").save(b, "JPEG", quality=a.quality, subsampling=a.subsampling, restart_marker_rows=1)
        return b.getvalue()

    files = [enc.encode(f)[0] for f in frames]
    same = all(x == host_file(f) for x, f in zip(files, frames))
    raw, packed = h * w * 3, statistics.mean(len(x) for x in files)
    print(f"{h}x{w} {a.subsampling} q{a.quality}: device files {'equal' if same else 'DIFFER FROM'} Pillow's; bytes to the host per "
          f"frame: raw {raw}, compressed {packed:.0f} ({raw / packed:.1f}x fewer); output reserved per frame {enc.capacity}")

    def launches():
        out, lengths, _, _ = next(x for x in enc._slots if x is not None)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(a.frames):
            enc.encode_into(frames[i % a.sets].unsqueeze(0), out[:1], lengths[:1])
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.frames * 1e3

    def pipeline():
        torch.cuda.synchronize()
        t = time.perf_counter()
        for i in range(a.frames):
            enc.submit(frames[i % a.sets])
            if i:
                enc.collect()
        enc.collect()
        return (time.perf_counter() - t) / a.frames * 1e6

    def host():
        torch.cuda.synchronize()
        t = time.perf_counter()
        for i in range(a.frames):
            host_file(frames[i % a.sets])
        return (time.perf_counter() - t) / a.frames * 1e6

    for what, fn in (("device, launches only (device events)", launches), ("device, to bytes on the host (wall clock)", pipeline),
                     ("host: raw copy + Image.save (wall clock)", host)):
        fn()
        us = [fn() for _ in range(a.samples)]
        print(f"{what}  us per frame: " + " ".join(f"{x:.0f}" for x in us) +
              f"  median {statistics.median(us):.0f} (min {min(us):.0f} max {max(us):.0f})")


if __name__ == "__main__":
    main()
