"""Writes the goldens of the frame-scaling tests (tests/test_scale_cpu.py, tests/test_scale_gpu.py):

  scale_cases.npz         small uint8 sources, the transform parameters and what Pillow makes of them with
                          Image.resize(BICUBIC) -> crop (the reference's rule) -> transpose(FLIP_LEFT_RIGHT); the Pillow
                          version is recorded
  img_params_cases.json   results of the reference's own data.transform.get_img_params under fixed seeds
                          (needs --reference DIR, the reference checkout; torchvision is stubbed for the import)

    python tests/golden/make_scale_goldens.py --reference /path/to/reference

Needs Pillow; the tests that read these files do not.  Without --reference only the .npz is written.
"""
import argparse
import json
import os
import random
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

# name, source (h, w), scaled (H, W), crop_size (w, h), crop_pos (x, y), flip, source kind, frames
CASES = [
    ("up_dword", (37, 53), (64, 96), (0, 0), (0, 0), False, "rand", 1),
    ("up_scalar", (37, 53), (63, 95), (0, 0), (0, 0), False, "rand", 1),
    ("down_9_7_taps", (64, 96), (32, 64), (0, 0), (0, 0), False, "rand", 1),
    ("down_33_taps", (50, 70), (13, 9), (0, 0), (0, 0), False, "rand", 1),
    ("down_to_1x1", (50, 70), (1, 1), (0, 0), (0, 0), False, "rand", 1),
    ("narrow_source", (9, 11), (64, 128), (0, 0), (0, 0), False, "rand", 1),
    ("from_1x1", (1, 1), (8, 12), (0, 0), (0, 0), False, "rand", 1),
    ("skip_vertical", (33, 47), (33, 96), (0, 0), (0, 0), False, "rand", 1),
    ("skip_horizontal", (33, 47), (64, 47), (0, 0), (0, 0), False, "rand", 1),
    ("skip_both", (33, 47), (33, 47), (0, 0), (0, 0), False, "rand", 1),
    ("crop", (64, 96), (80, 120), (64, 64), (16, 8), False, "rand", 1),
    ("crop_off_edge", (64, 96), (80, 120), (64, 64), (70, 40), False, "rand", 1),
    ("crop_larger_than_image", (64, 96), (80, 120), (128, 128), (5, 3), False, "rand", 1),
    ("flip", (64, 96), (80, 120), (0, 0), (0, 0), True, "rand", 1),
    ("flip_crop", (64, 96), (80, 120), (64, 64), (16, 8), True, "rand", 1),
    ("skip_both_flip_crop", (33, 47), (33, 47), (32, 16), (7, 5), True, "rand", 1),
    ("checker_down", (63, 95), (37, 53), (0, 0), (0, 0), False, "checker", 1),
    ("checker_up", (37, 53), (64, 96), (0, 0), (0, 0), False, "checker", 1),
    ("steps_down", (63, 95), (37, 53), (0, 0), (0, 0), False, "steps", 1),
    ("steps_up", (37, 53), (64, 96), (0, 0), (0, 0), False, "steps", 1),
]
SATURATING = ("checker_down", "checker_up", "steps_down", "steps_up")


def source(kind, n, h, w, c, rng):
    if kind == "rand":
        return rng.integers(0, 256, (n, h, w, c), dtype=np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    if kind == "checker":                       # 0 / 255 squares of 4, 7 and 3 pixels, one size per channel
        planes = [(((y // s) + (x // s)) % 2 * 255) for s in (4, 7, 3)]
    else:                                        # step edges: vertical, horizontal, diagonal
        planes = [(x >= w // 2) * 255, (y >= h // 3) * 255, ((x + y) % 11 >= 5) * 255]
    img = np.stack(planes[:c], -1).astype(np.uint8)
    return np.repeat(img[None], n, 0)


def pillow_transform(frame, scaled_hw, crop_size, crop_pos, flip):
    from PIL import Image
    h, w, c = frame.shape
    img = Image.fromarray(frame[..., 0] if c == 1 else frame)
    img = img.resize((scaled_hw[1], scaled_hw[0]), Image.BICUBIC)
    ow, oh = img.size
    (tw, th), (x1, y1) = crop_size, crop_pos
    if (tw, th) != (0, 0) and (ow > tw or oh > th):
        img = img.crop((x1, y1, min(ow, x1 + tw), min(oh, y1 + th)))
    if flip:
        img = img.transpose(Image.FLIP_LEFT_RIGHT)
    out = np.asarray(img)
    return out.reshape(out.shape[0], out.shape[1], c)


def write_scale_cases(path):
    import PIL
    rng = np.random.default_rng(20260)
    arrays, meta = {}, []
    for name, (h, w), (H, W), crop_size, crop_pos, flip, kind, n in CASES:
        for c in (1, 3):
            src = source(kind, n, h, w, c, rng)
            arrays[f"{name}/c{c}/src"] = src
            arrays[f"{name}/c{c}/out"] = np.stack([pillow_transform(f, (H, W), crop_size, crop_pos, flip) for f in src])
        meta.append({"name": name, "src_hw": [h, w], "new_size": [W, H], "crop_size": list(crop_size), "crop_pos": list(crop_pos),
                     "flip": flip, "kind": kind, "frames": n, "saturating": name in SATURATING})
    arrays["cases"] = np.array(json.dumps(meta))
    arrays["pillow_version"] = np.array(PIL.__version__)
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes, Pillow", PIL.__version__)


def write_img_params(path, reference):
    sys.modules.setdefault("torchvision", types.ModuleType("torchvision"))
    sys.modules.setdefault("torchvision.transforms", types.ModuleType("torchvision.transforms"))
    sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
    sys.path.insert(0, reference)
    from data.transform import get_img_params
    records = []
    seed = 1000
    for size in ((640, 512), (320, 256), (517, 389)):
        for scale in ("resize", "scale-width", "scale-height", "random-scale-width"):
            for crop in ("none", "crop", "scaled-crop"):
                for load_size, fine_size, mode in ((1024, 512, "ir2rgb"), (286, 256, "ir2rgb"), (600, 330, "pose")):
                    for _ in range(2):
                        seed += 1
                        opt = {"dataset_scale": scale, "dataset_crop": crop, "load_size": load_size, "fine_size": fine_size,
                               "dataset_mode": mode}
                        random.seed(seed)
                        np.random.seed(seed)
                        p = get_img_params(size, **opt)
                        records.append({"size": list(size), "seed": seed, "opt": opt,
                                        "new_size": [int(v) for v in p["new_size"]], "crop_size": [int(v) for v in p["crop_size"]],
                                        "crop_pos": [int(v) for v in p["crop_pos"]], "flip": bool(p["flip"])})
    with open(path, "w") as f:
        f.write('{"source": "data.transform.get_img_params of the reference, random.seed(seed) and np.random.seed(seed) per record",\n'
                ' "records": [\n')
        f.write(",\n".join("  " + json.dumps(r) for r in records))         # one record per line
        f.write("\n ]}\n")
    print(path, len(records), "records")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=None, help="checkout of the reference (for img_params_cases.json)")
    a = ap.parse_args()
    write_scale_cases(os.path.join(HERE, "scale_cases.npz"))
    if a.reference:
        write_img_params(os.path.join(HERE, "img_params_cases.json"), a.reference)
