"""Generates tests/golden/visuals_tensor2im.npz and visuals_panels.npz from the REFERENCE's own util/util.py.

Runs in the authoring container only (the reference is importable there; it never travels to the GPU box).  OpenCV is not
installed, and util.util imports it at the top: an empty stand-in module named ``cv2`` goes into ``sys.modules`` first, the
way make_window_goldens.py stubs the CUDA extensions.  Nothing that needs cv2 is recorded: ``tensor2flow`` is replaced by a
marker while ``save_all_tensors`` runs, so the flow coding is NOT pinned by these files (ir2rgb_amd/visuals.py says what
pins it instead).  Stored: inputs and outputs only.

* visuals_tensor2im.npz   ``tensor2im`` with normalize True / False on 5-D [2,2,C,5,7], 4-D and 3-D tensors with one and
  three channels (random values reaching below -1 and above 1), and on ``boundary`` inputs: every k/255 and 2k/255 - 1 for
  k = 0..255 with its fp32 neighbours below and above, where truncation and rounding part.
* visuals_panels.npz      ``save_all_tensors`` for input_nc 1 and 3, with and without a generator flow: the ordered names
  and every non-flow array; the inputs.
"""
import os
import sys
import types

import numpy as np
import torch

sys.modules.setdefault("cv2", types.ModuleType("cv2"))
sys.path.insert(0, "/root/reference")
from util import util as ref_util  # noqa: E402  (the reference)

HERE = os.path.dirname(os.path.abspath(__file__))
FLOW_MARKER = "tensor2flow"


def boundary_values():
    k = np.arange(256, dtype=np.float64)
    vals = []
    for base in (k / 255.0, 2.0 * k / 255.0 - 1.0):
        b = base.astype(np.float32)
        vals += [b, np.nextafter(b, np.float32(-4)), np.nextafter(b, np.float32(4))]
    v = np.concatenate(vals + [np.array([-1.5, -1.0000001, 1.0000001, 1.5, 2.0, -0.0, 0.0], dtype=np.float32)])
    pad = (-len(v)) % 21
    return np.concatenate([v, np.zeros(pad, dtype=np.float32)]).astype(np.float32)


def tensor2im_cases():
    g = torch.Generator().manual_seed(1234)
    out = {}
    for c in (1, 3):
        for shape in ((2, 2, c, 5, 7), (2, c, 5, 7), (c, 5, 7)):
            x = torch.randn(shape, generator=g) * 0.9            # (about a quarter of the values outside [-1, 1])
            x.view(-1)[:4] = torch.tensor([-1.75, 1.75, -1.0, 1.0])
            key = f"rand_c{c}_d{len(shape)}"
            out[key + "/x"] = x.numpy()
            out[key + "/norm"] = ref_util.tensor2im(x)
            out[key + "/unit"] = ref_util.tensor2im(x, normalize=False)
    b = boundary_values()
    for c in (1, 3):
        x = torch.from_numpy(b.reshape(c, -1, 7))
        key = f"boundary_c{c}"
        out[key + "/x"] = x.numpy()
        out[key + "/norm"] = ref_util.tensor2im(x)
        out[key + "/unit"] = ref_util.tensor2im(x, normalize=False)
    return out


def panel_cases():
    g = torch.Generator().manual_seed(4321)
    out = {}
    real_tensor2flow = ref_util.tensor2flow
    ref_util.tensor2flow = lambda output, imtype=np.uint8: FLOW_MARKER
    try:
        for input_nc in (1, 3):
            for with_flow in (False, True):
                r = lambda *s: torch.randn(s, generator=g) * 0.8  # noqa: E731
                t = dict(real_A=r(1, 2, input_nc, 5, 7), fake_B=r(1, 2, 3, 5, 7), fake_B_first=r(3, 5, 7), fake_B_raw=r(1, 2, 3, 5, 7),
                         real_B=r(1, 2, 3, 5, 7), flow_ref=r(1, 2, 2, 5, 7), conf_ref=torch.rand((1, 2, 1, 5, 7), generator=g),
                         flow=r(1, 2, 2, 5, 7) if with_flow else None,
                         weight=torch.rand((1, 2, 1, 5, 7), generator=g) if with_flow else None)
                opt = types.SimpleNamespace(label_nc=0, dataset_mode="ir2rgb", input_nc=input_nc, add_face_disc=False)
                visuals = ref_util.save_all_tensors(opt, t["real_A"], t["fake_B"], t["fake_B_first"], t["fake_B_raw"], t["real_B"],
                                                    t["flow_ref"], t["conf_ref"], t["flow"], t["weight"], None)
                key = f"nc{input_nc}_flow{int(with_flow)}"
                out[key + "/names"] = np.array(list(visuals.keys()))
                out[key + "/flow_names"] = np.array([k for k, v in visuals.items() if isinstance(v, str) and v == FLOW_MARKER])
                for k, v in t.items():
                    if v is not None:
                        out[f"{key}/in/{k}"] = v.numpy()
                for k, v in visuals.items():
                    if not isinstance(v, str):
                        out[f"{key}/out/{k}"] = v
    finally:
        ref_util.tensor2flow = real_tensor2flow
    return out


if __name__ == "__main__":
    np.savez_compressed(os.path.join(HERE, "visuals_tensor2im.npz"), **tensor2im_cases())
    np.savez_compressed(os.path.join(HERE, "visuals_panels.npz"), **panel_cases())
    print("wrote visuals_tensor2im.npz, visuals_panels.npz")
