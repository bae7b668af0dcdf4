"""JPEG files of camera frames: decoded on the device (ir2rgb_amd.JpegDecoder, csrc/jpeg_decode.hip) beside what the host
does today, in one process:

    python tools/microbench/jpeg_decode_bench.py [--height 512] [--width 640] [--frames 50] [--samples 5] [--chunk 16]

For 4:2:0 files of quality 75 and 90, without and with restart markers (``restart_marker_rows=1``), ``--frames`` files
(``--sets`` different ones taken in turn: smooth colour with noise, the content of the full-size golden) go through

  device, launches only   the three launches of ir2rgb_jpeg_decode_u8 on ``--chunk`` staged files between two device
                          events, for every ``--sub-bytes`` value (the table DEFAULT_SUB_BYTES was chosen from)
  device, from bytes      submit(chunk k + 1) / collect(chunk k): header parsing on the host, one pinned upload, the launches,
                          the status copy -- to a finished uint8 device tensor (wall clock, the pipeline
                          JpegDecoder.frames runs)
  host                    Image.open + np.asarray on one core, then the upload of the pixels (wall clock)

and the relaxation rounds the entropy kernel took per file and the bytes that cross to the device are printed.  The pixels
of the two paths are compared once."""
import argparse
import io
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "tests", "golden"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from ir2rgb_amd.jpeg_decode import DEFAULT_SUB_BYTES, JpegDecoder  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--sets", type=int, default=8)
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--subsampling", default="4:2:0")
    ap.add_argument("--sub-bytes", type=int, nargs="*", default=[32, 64, 128, 256, 512])
    a = ap.parse_args()
    assert torch.cuda.is_available(), "jpeg_decode_bench needs the GPU"
    from PIL import Image
    from make_jpeg_decode_goldens import content
    dev = torch.device("cuda:0")
    h, w = a.height, a.width
    sources = [content("smooth", h, w, 500 + s) for s in range(a.sets)]
    pinned = torch.empty((h, w, 3), dtype=torch.uint8, pin_memory=True)
    on_device = torch.empty((h, w, 3), dtype=torch.uint8, device=dev)

    def host_frame(data):
        pinned.copy_(torch.from_numpy(np.asarray(Image.open(io.BytesIO(data)))))
        on_device.copy_(pinned, non_blocking=True)
        return on_device

    def median(fn):
        fn()
        us = [fn() for _ in range(a.samples)]
        return f"median {statistics.median(us):.0f} (min {min(us):.0f} max {max(us):.0f})"

    for quality in (75, 90):
        for restart_rows in (0, 1):
            files = []
            for src in sources:
                b = io.BytesIO()
                Image.fromarray(src).save(b, "JPEG", quality=quality, subsampling=a.subsampling, restart_marker_rows=restart_rows)
                files.append(b.getvalue())
            dec = JpegDecoder.for_file(dev, files[0])
            got = dec.decode(files)
            rounds = dec.rounds()
            same = all(torch.equal(got[i], host_frame(f)) for i, f in enumerate(files))
            size = statistics.mean(len(f) for f in files)
            print(f"== {h}x{w} {a.subsampling} q{quality} restart_marker_rows={restart_rows}: device pixels "
                  f"{'equal' if same else 'DIFFER FROM'} Pillow's; bytes to the device per frame: pixels {h * w * 3}, file {size:.0f} "
                  f"({h * w * 3 / size:.1f}x fewer); segments per file {rounds.shape[1]}; rounds per file (most over its segments) "
                  f"{rounds.max(axis=1).tolist()}")
            batch = [files[i % a.sets] for i in range(a.chunk)]
            infos, _ = dec.prepare(batch)
            block, n_seg, layout = dec.pack(infos)
            staged = torch.from_numpy(block).to(dev)
            out = torch.empty((a.chunk, h, w, dec.C), dtype=torch.uint8, device=dev)
            status = torch.empty(a.chunk, dtype=torch.int32, device=dev)
            calls = max(a.frames // a.chunk, 1)

            def launches(sub):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(calls):
                    dec.decode_into(staged, a.chunk, n_seg, layout, out, status, sub_bytes=sub)
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) / (calls * a.chunk) * 1e3

            for sub in a.sub_bytes:
                print(f"device, launches only, {a.chunk} files per call, sub_bytes {sub:4d}  us per frame: " + median(lambda: launches(sub)))
            order = [files[i % a.sets] for i in range(a.frames)]

            def pipeline():
                torch.cuda.synchronize()
                t = time.perf_counter()
                n = sum(1 for _ in dec.frames(order, chunk=a.chunk))
                torch.cuda.synchronize()
                assert n == a.frames
                return (time.perf_counter() - t) / a.frames * 1e6

            def host():
                torch.cuda.synchronize()
                t = time.perf_counter()
                for f in order:
                    host_frame(f)
                torch.cuda.synchronize()
                return (time.perf_counter() - t) / a.frames * 1e6

            print(f"device, from bytes to a device tensor (wall clock, sub_bytes {DEFAULT_SUB_BYTES})  us per frame: " + median(pipeline))
            print("host: Image.open + np.asarray + upload (wall clock)  us per frame: " + median(host))


if __name__ == "__main__":
    main()
