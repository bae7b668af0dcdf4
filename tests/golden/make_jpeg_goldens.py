"""Writes tests/golden/jpeg_cases.npz, the goldens of the JPEG tests (tests/test_jpeg_cpu.py, tests/test_jpeg_gpu.py): the
files Pillow writes with ``Image.save(f, "JPEG", quality=q, subsampling=..., restart_marker_rows=r)``.

    python tests/golden/make_jpeg_goldens.py

  grid      SHAPES x the three modes x QUALITIES x RESTART_ROWS on one source per shape (noise over a gradient); mode L
            takes channel 0.  144x40 has more than 8 intervals, so the RST index wraps.
  extras    content chosen for one path each: saturated checkerboards at q = 100 (DC size 11, AC size 10), a flat
            frame (blocks that are one EOB), sparse noise (ZRL), and 16x344, whose intervals are longer than the 128 blocks
            the entropy kernel takes at a time
  fullsize  one 512x1024 frame per mode, made by ``fullsize_frame`` from a seed: SHA-256 and length of Pillow's file

The files are stored as bytes in one array (``files``, with offset and length per case).  Needs Pillow on libjpeg-turbo;
the tests that read the file do not.  This module is also where the tests take ``source`` and ``fullsize_frame`` from.
"""
import hashlib
import io
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "jpeg_cases.npz")

SHAPES = [(1, 1), (8, 8), (8, 24), (24, 8), (7, 9), (13, 21), (16, 16), (17, 33), (31, 47), (144, 40)]
MODES = ("4:4:4", "4:2:0", "L")
QUALITIES = (1, 30, 75, 95, 100)
RESTART_ROWS = (1, 2)
# name, (H, W), content, quality
EXTRAS = [("checker", (16, 16), "checker", 100), ("checker_odd", (17, 33), "checker", 100), ("flat", (17, 33), "flat", 75),
          ("sparse", (31, 47), "sparse", 95), ("long_interval", (16, 344), "noise", 75)]
FULLSIZE = (512, 1024)
FULLSIZE_SEED = 2026


def source(kind, h, w, seed):
    """uint8 [h, w, 3]."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    if kind == "checker":       # blocks in turn 0 / 255 by pixel, white, black: the largest AC coefficients and DC steps there are
        which = (y // 8 + x // 8) % 3
        v = np.where(which == 0, (y + x) % 2 * 255, np.where(which == 1, 255, 0))
        return np.repeat(v[..., None], 3, -1).astype(np.uint8)
    if kind == "flat":
        return np.full((h, w, 3), (200, 31, 97), dtype=np.uint8)
    if kind == "sparse":                                        # a few bright pixels on black: long zero runs between coefficients
        a = np.zeros((h, w, 3), dtype=np.uint8)
        a[rng.random((h, w)) < 0.04] = (255, 160, 40)
        return a
    grad = np.stack([(3 * y + 2 * x) % 256, (5 * y + x) % 256, (2 * y + 7 * x) % 256], -1)
    noise = rng.integers(-48, 49, (h, w, 3))
    return np.clip(grad + noise, 0, 255).astype(np.uint8)


def fullsize_frame(seed=FULLSIZE_SEED, hw=FULLSIZE):
    """The full-size frame of the ``fullsize`` goldens: smooth colour, noise in a band, flat saturated patches."""
    h, w = hw
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    a = np.stack([(y // 2 + x // 4) % 256, (y + x // 3) % 256, (255 - y // 3 + x // 5) % 256], -1)
    a[h // 4:h // 2] += rng.integers(-40, 41, (h // 2 - h // 4, w, 3))
    a = np.clip(a, 0, 255).astype(np.uint8)
    a[h // 8:h // 6, w // 8:w // 2] = 255
    a[3 * h // 4:7 * h // 8, w // 2:] = 0
    return a


def pillow_file(frame, mode, quality, restart_rows):
    from PIL import Image
    b = io.BytesIO()
    if mode == "L":
        Image.fromarray(np.ascontiguousarray(frame[..., 0]), "L").save(b, "JPEG", quality=quality, restart_marker_rows=restart_rows)
    else:
        Image.fromarray(frame, "RGB").save(b, "JPEG", quality=quality, subsampling=mode, restart_marker_rows=restart_rows)
    return b.getvalue()


def main():
    import PIL
    from PIL import features
    assert features.check_feature("libjpeg_turbo"), "the goldens are libjpeg-turbo's files"
    arrays, meta, files, offset = {}, [], [], 0

    def add(name, src_key, frame, mode, q, rr):
        nonlocal offset
        data = pillow_file(frame, mode, q, rr)
        meta.append({"name": name, "src": src_key, "hw": list(frame.shape[:2]), "mode": mode, "quality": q, "restart_rows": rr,
                     "offset": offset, "length": len(data)})
        files.append(np.frombuffer(data, dtype=np.uint8))
        offset += len(data)

    for i, (h, w) in enumerate(SHAPES):
        key = f"src/{h}x{w}"
        arrays[key] = source("noise", h, w, 100 + i)
        for mode in MODES:
            for q in QUALITIES:
                for rr in RESTART_ROWS:
                    add(f"{h}x{w}/{mode}/q{q}/r{rr}", key, arrays[key], mode, q, rr)
    for i, (name, (h, w), kind, q) in enumerate(EXTRAS):
        key = f"src/{name}"
        arrays[key] = source(kind, h, w, 200 + i)
        for mode in MODES:
            for rr in RESTART_ROWS:
                add(f"{name}/{mode}/q{q}/r{rr}", key, arrays[key], mode, q, rr)
    full = []
    frame = fullsize_frame()
    for mode in MODES:
        data = pillow_file(frame, mode, 75, 1)
        full.append({"mode": mode, "quality": 75, "restart_rows": 1, "seed": FULLSIZE_SEED, "hw": list(FULLSIZE),
                     "sha256": hashlib.sha256(data).hexdigest(), "length": len(data)})
    arrays["files"] = np.concatenate(files)
    arrays["cases"] = np.array(json.dumps(meta))
    arrays["fullsize"] = np.array(json.dumps(full))
    arrays["pillow_version"] = np.array(f"{PIL.__version__} libjpeg-turbo {features.version_feature('libjpeg_turbo')}")
    np.savez_compressed(PATH, **arrays)
    print(PATH, os.path.getsize(PATH), "bytes,", len(meta), "cases, Pillow", arrays["pillow_version"])


if __name__ == "__main__":
    main()
