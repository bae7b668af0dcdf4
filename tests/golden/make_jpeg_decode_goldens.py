"""Writes the fixtures of the JPEG decoder tests (tests/test_jpeg_decode_cpu.py, tests/test_jpeg_decode_gpu.py):

  jpeg_decode_cases.npz    files written by Pillow (Image.save(..., "JPEG", quality, subsampling, optimize,
                           restart_marker_rows)) and the pixels Pillow decodes from them, np.asarray(Image.open(f)); one
                           512x640 file per mode without restart markers as bytes + SHA-256 of the pixels
  video_params_cases.json  results of the reference's own data.transform.get_video_params under fixed seeds
                           (needs --reference DIR, the reference checkout; torchvision is stubbed for the import)

    python tests/golden/make_jpeg_decode_goldens.py --reference /path/to/reference

Needs Pillow; the tests that read these files do not.  It ends by checking that the cases reach every rule of the
definition (the COUNTERS of ir2rgb_amd.jpeg_decode).
"""
import argparse
import hashlib
import io
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
PATH = os.path.join(HERE, "jpeg_decode_cases.npz")
PARAMS = os.path.join(HERE, "video_params_cases.json")

SHAPES = ((1, 1), (2, 3), (5, 4), (8, 8), (9, 17), (17, 33), (31, 47), (40, 24), (64, 80))
MODES = ("4:4:4", "4:2:2", "4:2:0", "L")
QUALITIES = (1, 30, 75, 95, 100)
CONTENTS = ("smooth", "noise", "checker", "flat")
FORCED_SUB_BYTES = (4, 16, 64)          # what the tests force besides the default


def content(kind, h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "smooth":
        a = np.stack([127 + 110 * np.sin(xx / 7 + yy / 5), 127 + 110 * np.cos(xx / 3 - yy / 9), 127 + 90 * np.sin(yy / 4)], -1)
        a = a + rng.normal(0, 10, (h, w, 3))
    elif kind == "noise":
        a = rng.integers(0, 256, (h, w, 3))
    elif kind == "checker":
        a = ((((xx + yy) & 1) * 255)[..., None] ^ np.array([0, 255, 0])[None, None, :])
    else:
        a = np.full((h, w, 3), 77)
    return np.clip(a, 0, 255).astype(np.uint8)


def pillow_file(frame, mode, quality, optimize, restart_rows):
    from PIL import Image
    buf = io.BytesIO()
    kw = {} if mode == "L" else dict(subsampling=mode)
    Image.fromarray(frame[..., 0] if mode == "L" else frame).save(buf, "JPEG", quality=quality, optimize=optimize,
                                                                  restart_marker_rows=restart_rows, **kw)
    data = buf.getvalue()
    return data, np.asarray(Image.open(io.BytesIO(data)))


def case_list():
    """(name, (h, w), content, mode, quality, optimize, restart_rows): every shape x mode x quality, the contents and options
    taking turns; then the extras."""
    cases, turn = [], 0
    for h, w in SHAPES:
        for mode in MODES:
            for q in QUALITIES:
                kind = CONTENTS[turn % 3]                                  # smooth, noise, checker
                cases.append((f"{h}x{w}/{mode}/q{q}", (h, w), kind, mode, q, turn % 5 == 2, (0, 1, 2)[(turn // 3) % 3]))
                turn += 1
    for mode in MODES:
        cases.append((f"flat/{mode}", (24, 40), "flat", mode, 75, False, 0))
        cases.append((f"dw3/{mode}", (7, 5), "smooth", mode, 95, False, 0))                  # the narrowest fancy upsampling
        cases.append((f"tall/{mode}", (88, 12), "noise", mode, 95, mode == "4:2:0", 1))      # more than 8 intervals
        cases.append((f"long/{mode}", (48, 112), "noise", mode, 100, False, 0))              # sub_bytes 4 must be enlarged
    return cases


def fullsize_frame():
    return content("smooth", 512, 640, 99)


def write_cases(path):
    import PIL
    blobs, pixels, meta = [], [], []
    off = poff = 0
    for i, (name, hw, kind, mode, q, optimize, rr) in enumerate(case_list()):
        data, want = pillow_file(content(kind, *hw, seed=i), mode, q, optimize, rr)
        meta.append(dict(name=name, hw=list(hw), mode=mode, quality=q, optimize=optimize, restart_rows=rr, content=kind,
                         offset=off, length=len(data), pixel_offset=poff, shape=list(want.shape)))
        blobs.append(np.frombuffer(data, dtype=np.uint8))
        pixels.append(want.ravel())
        off, poff = off + len(data), poff + want.size
    full = []
    for mode in MODES:
        data, want = pillow_file(fullsize_frame(), mode, 75, False, 0)
        full.append(dict(mode=mode, offset=off, length=len(data), shape=list(want.shape),
                         sha256=hashlib.sha256(np.ascontiguousarray(want).tobytes()).hexdigest()))
        blobs.append(np.frombuffer(data, dtype=np.uint8))
        off += len(data)
    np.savez_compressed(path, files=np.concatenate(blobs), pixels=np.concatenate(pixels), cases=json.dumps(meta),
                        fullsize=json.dumps(full), pillow=PIL.__version__)
    print(path, len(meta), "cases +", len(full), "full-size files,", os.path.getsize(path), "bytes")


def load(path=PATH):
    """-> ([(meta, file bytes, pixels)], [(meta, file bytes)] of the full-size files)"""
    d = np.load(path)
    files, pixels = d["files"], d["pixels"]
    cases = [(m, files[m["offset"]:m["offset"] + m["length"]].tobytes(),
              pixels[m["pixel_offset"]:m["pixel_offset"] + int(np.prod(m["shape"]))].reshape(m["shape"]))
             for m in json.loads(str(d["cases"]))]
    full = [(m, files[m["offset"]:m["offset"] + m["length"]].tobytes()) for m in json.loads(str(d["fullsize"]))]
    return cases, full


def liveness(cases, full=()):
    """The COUNTERS of the definition over the committed cases: decode_reference of every file, and entropy_model at the
    forced subsequence sizes."""
    from ir2rgb_amd import jpeg_decode as D
    cnt = D._counters()
    for _, data, _ in cases:
        D.decode_reference(data, counters=cnt)
        info = D.parse(data)
        for sub in FORCED_SUB_BYTES:
            D.entropy_model(info, sub, counters=cnt)
    return cnt


def write_video_params(path, reference):
    sys.modules.setdefault("torchvision", types.ModuleType("torchvision"))
    sys.modules.setdefault("torchvision.transforms", types.ModuleType("torchvision.transforms"))
    sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
    sys.path.insert(0, reference)
    from data.transform import get_video_params
    records, seed = [], 2000
    for seq_len in (3, 6, 30, 128, 500):
        for n_frames_total in (1, 6, 30, 126):
            for max_frames_per_gpu, gen_gpus, batch_size in ((1, 1, 1), (2, 1, 1), (3, 2, 1), (3, 2, 2)):
                for max_t_step in (1, 4):
                    seed += 1
                    opt = dict(n_frames_total=n_frames_total, n_input_gen_frames=3, is_train=True, gen_gpus=gen_gpus,
                               batch_size=batch_size, max_frames_per_gpu=max_frames_per_gpu, max_t_step=max_t_step, debug=False)
                    np.random.seed(seed)
                    n, start, step = get_video_params(seq_len, 0, **opt)
                    records.append(dict(seq_len=seq_len, seed=seed, opt=opt, result=[int(n), int(start), int(step)]))
    with open(path, "w") as f:
        f.write('{"source": "data.transform.get_video_params of the reference, np.random.seed(seed) per record",\n "records": [\n')
        f.write(",\n".join("  " + json.dumps(r) for r in records))
        f.write("\n ]}\n")
    print(path, len(records), "records")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=None, help="checkout of the reference (for video_params_cases.json)")
    a = ap.parse_args()
    write_cases(PATH)
    if a.reference:
        write_video_params(PARAMS, a.reference)
    counters = liveness(load()[0])
    print(counters)
    dead = [k for k, v in counters.items() if not v]
    assert not dead, f"the cases never reach: {dead}"
