"""Frame scaling on the device: the reference loader's ``Image.resize(..., BICUBIC)``, crop and flip, bit for bit.

    get_img_params / get_transform / __scale_image / __crop / __flip          data/transform.py:13-113
    one parameter set per sequence                                            data/dataset/vid2vid.py:129-143

Pillow's 8-bit resampler (Resample.c) is fixed-point: per axis it computes, in double, a window ``[xmin, xmin + xmax)`` and
``xmax`` normalised bicubic weights for every output sample, converts each weight to an integer with 22 fraction bits, and
then evaluates ``clamp((2**21 + sum(px * k)) >> 22, 0, 255)`` in integers -- the horizontal pass first, rounded to uint8,
the vertical pass on those bytes.  Here the tables are computed on the host in Python floats (IEEE double) in Pillow's
operation order (``resample_coeffs``) and everything after them is integer arithmetic, in torch for the CPU oracle
(``resize_reference``) and in two HIP kernels (csrc/frame_scale.hip) for the device path (``FrameScaler``), so there is
nothing left that could round differently.

Sizes follow the reference's conventions: ``new_size`` / ``crop_size`` are (width, height) and ``crop_pos`` is (x, y), as
in the dict ``get_img_params`` returns; ``src_hw`` / ``out_hw`` are (rows, columns) like every tensor shape here.

Speed: not measured (tools/bench_infer.py has the rows).
"""
import math
import random as _random

import numpy as _np
import torch

from . import _lib

__all__ = ["resample_coeffs", "resize_reference", "transform_reference", "img_params", "output_window", "FrameScaler"]

PRECISION_BITS = 22


def _bicubic(x):
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def resample_coeffs(in_size, out_size):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for the bicubic filter over the whole axis -> (bounds, coeffs,
    ksize): ``bounds[xx] = (xmin, xmax)``, ``coeffs[xx]`` a list of ``ksize`` ints of which the first ``xmax`` count (the
    rest are 0).  Plain Python floats in Pillow's statement order."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError(f"resample_coeffs: sizes must be positive, got {in_size} -> {out_size}")
    scale = in_size / out_size
    filterscale = scale
    if filterscale < 1.0:
        filterscale = 1.0
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    bounds, coeffs = [], []
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = int(center - support + 0.5)
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        xmax -= xmin
        k, ww = [], 0.0
        for x in range(xmax):
            w = _bicubic((x + xmin - center + 0.5) * ss)
            k.append(w)
            ww += w
        if ww != 0.0:
            k = [w / ww for w in k]
        row = [int(-0.5 + w * (1 << PRECISION_BITS)) if w < 0 else int(0.5 + w * (1 << PRECISION_BITS)) for w in k]
        bounds.append((xmin, xmax))
        coeffs.append(row + [0] * (ksize - xmax))
    return bounds, coeffs, ksize


def _pass(img, axis, out_size):
    """One resampling pass along ``axis`` of a uint8 tensor: int32 sums, arithmetic shift, clamp, back to uint8."""
    in_size = img.shape[axis]
    bounds, coeffs, ksize = resample_coeffs(in_size, out_size)
    dev = img.device
    xmin = torch.tensor([b[0] for b in bounds], dtype=torch.long, device=dev)
    k = torch.tensor(coeffs, dtype=torch.int32, device=dev)
    shape = [1] * img.dim()
    shape[axis] = out_size
    src = img.to(torch.int32)
    acc = torch.full([out_size if d == axis else s for d, s in enumerate(img.shape)], 1 << (PRECISION_BITS - 1),
                     dtype=torch.int32, device=dev)
    for t in range(ksize):      # taps past xmax have coefficient 0; their (clamped) index reads a valid sample
        idx = (xmin + t).clamp_(max=in_size - 1)
        acc += src.index_select(axis, idx) * k[:, t].view(shape)
    return (acc >> PRECISION_BITS).clamp_(0, 255).to(torch.uint8)


def resize_reference(img_u8, new_size):
    """``PIL.Image.resize(new_size, BICUBIC)`` of uint8 ``[H,W,C]`` (or ``[N,H,W,C]``, ``[H,W]``) as integer torch code on
    the tensor's device: the CPU oracle of the kernels.  ``new_size`` = (width, height).  The horizontal pass runs first
    and is rounded to uint8; a pass whose size does not change is skipped."""
    img = torch.as_tensor(img_u8)
    if img.dtype != torch.uint8:
        raise TypeError(f"resize_reference: uint8 expected, got {img.dtype}")
    squeeze = img.dim() == 2
    if squeeze:
        img = img.unsqueeze(-1)
    if img.dim() not in (3, 4):
        raise ValueError(f"resize_reference: [H,W,C] or [N,H,W,C] expected, got {tuple(img.shape)}")
    new_w, new_h = int(new_size[0]), int(new_size[1])
    ax_h, ax_w = img.dim() - 3, img.dim() - 2
    out = img
    if new_w != img.shape[ax_w]:
        out = _pass(out, ax_w, new_w)
    if new_h != img.shape[ax_h]:
        out = _pass(out, ax_h, new_h)
    if out is img:
        out = img.clone()
    return out.squeeze(-1) if squeeze else out


def output_window(new_size, crop_size=(0, 0), crop_pos=(0, 0)):
    """The reference's ``__crop`` on an image of ``new_size``: -> (crop_x, crop_y, out_w, out_h).  The crop applies only if
    ``ow > tw or oh > th`` and is clamped to the image at the right and bottom edge."""
    ow, oh = int(new_size[0]), int(new_size[1])
    tw, th = int(crop_size[0]), int(crop_size[1])
    x1, y1 = int(crop_pos[0]), int(crop_pos[1])
    if tw > 0 and th > 0 and (ow > tw or oh > th):
        x2, y2 = min(ow, x1 + tw), min(oh, y1 + th)
        if x1 < 0 or y1 < 0 or x2 <= x1 or y2 <= y1:
            raise ValueError(f"crop {crop_size} at {crop_pos} leaves nothing of a {ow}x{oh} image")
        return x1, y1, x2 - x1, y2 - y1
    return 0, 0, ow, oh


def transform_reference(img_u8, new_size, crop_size=(0, 0), crop_pos=(0, 0), flip=False):
    """scale -> crop -> flip of uint8 ``[H,W,C]`` / ``[N,H,W,C]`` with ``resize_reference``: what ``FrameScaler`` computes."""
    out = resize_reference(img_u8, new_size)
    x, y, w, h = output_window(new_size, crop_size, crop_pos)
    ax = out.dim() - 3
    out = out.narrow(ax, y, h).narrow(ax + 1, x, w)
    if flip:
        out = out.flip(ax + 1)
    return out.contiguous()


def _make_power_2(n, base=32.0):
    return int(round(n / base) * base)


_SCALES = ("resize", "scale-width", "scale-height", "random-scale-width", "none")
_CROPS = ("none", "crop", "scaled-crop")


def img_params(size, rng=None, **opt):
    """The parameter set of one sequence, as the reference's ``get_img_params`` chooses it.  ``size`` = (width, height) of
    the camera frame.  Options (the reference's names): ``dataset_scale``, ``dataset_crop``, ``load_size``, ``fine_size``,
    ``dataset_mode``, ``is_train``, ``flip``.  ``rng`` = (random-like, numpy.random-like) sources; the default is the
    ``random`` module and ``numpy.random``, drawn from in the reference's order (randint for a random scale, randn for
    crop_x, randint for crop_y, random for flip), so a seeded run reproduces the reference's choice.

    -> dict with the reference's keys ``new_size``, ``crop_size``, ``crop_pos`` (all (w, h) / (x, y)) and ``flip`` (the
    draw), plus what ``get_transform`` makes of them: ``scale_size`` (``load_size x load_size`` for ``resize`` whatever
    ``new_size`` says), ``apply_crop`` and ``apply_flip`` (the draw counts only with ``is_train and flip``).

    Kept quirks: sizes are rounded to a multiple of 4 and to a multiple of 32 only when nothing is cropped; both crop
    modes take ``fine_size x fine_size``.  ``dataset_scale='none'`` (an AttributeError in the reference) is the size
    unchanged, then the same rounding; ``'random-scale-height'`` (also an AttributeError there) raises ValueError."""
    py, npr = rng if rng is not None else (_random, _np.random)
    scale, crop = opt.get("dataset_scale", "none"), opt.get("dataset_crop", "none")
    if scale == "random-scale-height":
        raise ValueError("dataset_scale='random-scale-height' raises AttributeError in the reference (get_img_params reads "
                         "kwargs.dataset_scale on a dict), so it has no behaviour to reproduce")
    if scale not in _SCALES:
        raise ValueError(f"dataset_scale: one of {_SCALES}, got {scale!r}")
    if crop not in _CROPS:
        raise ValueError(f"dataset_crop: one of {_CROPS}, got {crop!r}")
    w, h = int(size[0]), int(size[1])
    new_h, new_w = h, w
    if scale == "resize":
        new_h = new_w = opt["load_size"]
    elif scale == "scale-width":
        new_w = opt["load_size"]
        new_h = opt["load_size"] * h // w
    elif scale == "scale-height":
        new_h = opt["load_size"]
        new_w = opt["load_size"] * w // h
    elif scale == "random-scale-width":
        new_w = py.randint(opt["fine_size"], opt["load_size"] + 1)
        new_h = new_w * h // w
    new_w = int(round(new_w / 4)) * 4
    new_h = int(round(new_h / 4)) * 4
    crop_x = crop_y = crop_w = crop_h = 0
    if crop != "none":
        crop_w = crop_h = _make_power_2(opt["fine_size"])       # 'crop' is part of both mode names
        x_span = (new_w - crop_w) // 2
        crop_x = int(max(0, min(x_span * 2, int(npr.randn() * x_span / 3 + x_span))))
        crop_y = int(py.randint(0, int(min(max(0, new_h - crop_h), new_h // 8))))
    else:
        new_w, new_h = _make_power_2(new_w), _make_power_2(new_h)
    flip = bool(py.random() > 0.5) and opt.get("dataset_mode") != "pose"
    scale_size = (int(opt["load_size"]),) * 2 if scale == "resize" else (new_w, new_h)
    return {"new_size": (new_w, new_h), "crop_size": (crop_w, crop_h), "crop_pos": (crop_x, crop_y), "flip": flip,
            "scale_size": scale_size, "apply_crop": crop != "none",
            "apply_flip": bool(flip and opt.get("is_train") and opt.get("flip"))}


def _row_span(bounds, first, count):
    """Source rows [r0, r0 + rows) the outputs [first, first + count) of an axis read (both ends are monotonic)."""
    r0 = bounds[first][0]
    last = bounds[first + count - 1]
    return r0, last[0] + last[1] - r0


class FrameScaler:
    """Scale -> crop -> flip of uint8 frames on the device (csrc/frame_scale.hip), equal to Pillow's bicubic ``resize``,
    ``crop`` and ``transpose(FLIP_LEFT_RIGHT)`` byte for byte.  The coefficient tables are uploaded once.  The workspace (the
    horizontally scaled rows the kept output rows read) of ONE frame is owned here and lives, at one address, as long as
    the scaler does -- a captured graph may hold that address; a call with a larger batch takes a temporary of its own and
    leaves the owned buffer alone.  Calls on one scaler share that buffer, so they belong on one stream (``clone()`` gives
    a scaler with the same tables and a workspace of its own).

        sc = FrameScaler(dev, (512, 640), 3, new_size=(1024, 832))
        sc.out_hw                                     # (832, 1024)
        rgb = sc(frames_u8)                           # uint8 [N,832,1024,3]  (or [832,1024,3] for one frame)
        x = sc(frames_u8, normalised=True)            # fp32 [N,3,832,1024] = inference.normalise_u8 of the above

    A call enqueues two launches on the current stream and does not synchronise with the host."""

    def __init__(self, device, src_hw, channels, new_size, crop_size=(0, 0), crop_pos=(0, 0), flip=False):
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError("FrameScaler runs on an AMD GPU only (ir2rgb_amd has no CPU fallback; resize_reference is the CPU oracle)")
        self.device, self.channels = device, int(channels)
        self.src_hw = (int(src_hw[0]), int(src_hw[1]))
        self.new_size = (int(new_size[0]), int(new_size[1]))
        self.crop_size, self.crop_pos, self.flip = tuple(crop_size), tuple(crop_pos), bool(flip)
        if self.channels not in (1, 3):
            raise ValueError("FrameScaler: 1 or 3 channels")
        if min(self.src_hw + self.new_size) < 1:
            raise ValueError("FrameScaler: sizes must be positive")
        self.crop_x, self.crop_y, wc, hc = output_window(self.new_size, crop_size, crop_pos)
        self.out_hw = (hc, wc)
        self._geom = (self.channels, *self.src_hw, self.new_size[1], self.new_size[0], self.crop_y, self.crop_x, hc, wc)
        self.x_tables = self._upload(self.src_hw[1], self.new_size[0])
        self.y_tables = self._upload(self.src_hw[0], self.new_size[1])
        self._ws = torch.empty(self.workspace_bytes(1), dtype=torch.uint8, device=self.device)      # never replaced

    def _upload(self, in_size, out_size):
        if in_size == out_size:
            return None, None, 0            # a skipped pass is a copy and reads no table
        bounds, coeffs, ksize = resample_coeffs(in_size, out_size)
        return (torch.tensor(bounds, dtype=torch.int32).to(self.device), torch.tensor(coeffs, dtype=torch.int32).to(self.device),
                ksize)

    def workspace_bytes(self, n=1):
        return int(_lib.query("ir2rgb_frame_scale_workspace_bytes", int(n), *self._geom))

    def _workspace(self, n):
        """-> (buffer, bytes needed) for a batch of ``n``: the owned one-frame buffer, or a temporary for this call alone
        (freed stream-ordered by the caching allocator) -- the owned buffer is never released or moved."""
        need = self.workspace_bytes(n)
        if need <= self._ws.numel():
            return self._ws, need
        return torch.empty(need, dtype=torch.uint8, device=self.device), need

    def clone(self):
        """The same transform on the same (read-only) tables with a workspace of its own."""
        import copy
        sc = copy.copy(self)
        sc._ws = torch.empty(self.workspace_bytes(1), dtype=torch.uint8, device=self.device)
        return sc

    def with_channels(self, channels):
        """The same transform for frames of another channel count (the RGB track beside a 1-channel IR track)."""
        if int(channels) == self.channels:
            return self
        return FrameScaler(self.device, self.src_hw, channels, self.new_size, self.crop_size, self.crop_pos, self.flip)

    @classmethod
    def from_options(cls, device, src_hw, channels, rng=None, **opt):
        """One parameter set chosen by ``img_params`` (call once per sequence) -> the scaler that applies it the way the
        reference's ``get_transform`` does."""
        p = img_params((src_hw[1], src_hw[0]), rng=rng, **opt)
        sc = cls(device, src_hw, channels, p["scale_size"], p["crop_size"] if p["apply_crop"] else (0, 0),
                 p["crop_pos"] if p["apply_crop"] else (0, 0), p["apply_flip"])
        sc.params = p
        return sc

    def __call__(self, frames_u8, out=None, normalised=False, workspace=None):
        """``frames_u8`` uint8 [Hs,Ws,C] or [N,Hs,Ws,C] on the device -> uint8 [N,Hc,Wc,C], or with ``normalised`` fp32
        [N,C,Hc,Wc] (ToTensor + Normalize(0.5, 0.5), bit-equal to ``inference.normalise_u8``); without the N axis for one
        frame.  ``out``: a contiguous tensor of that shape and dtype to write into (returned).  ``workspace``: a uint8 device
        buffer of at least ``workspace_bytes(N)`` bytes to use instead of the scaler's own."""
        _lib.require_device(frames_u8, out, self._ws, workspace)
        if frames_u8.dtype != torch.uint8:
            raise TypeError(f"FrameScaler: uint8 frames expected, got {frames_u8.dtype}")
        single = frames_u8.dim() == 3
        shape = tuple(frames_u8.shape[-3:])
        if frames_u8.dim() not in (3, 4) or shape != (*self.src_hw, self.channels):
            raise ValueError(f"FrameScaler: frames {tuple(frames_u8.shape)} given, [N,]{(*self.src_hw, self.channels)} expected")
        n = 1 if single else frames_u8.shape[0]
        if n < 1:
            raise ValueError("FrameScaler: an empty batch")
        hc, wc = self.out_hw
        want = (self.channels, hc, wc) if normalised else (hc, wc, self.channels)
        if not single:
            want = (n, *want)
        dtype = torch.float32 if normalised else torch.uint8
        if out is None:
            out = torch.empty(want, dtype=dtype, device=self.device)
        elif tuple(out.shape) != want or out.dtype != dtype:
            raise ValueError(f"FrameScaler: out {tuple(out.shape)} {out.dtype} given, {want} {dtype} expected")
        if workspace is None:
            ws, need = self._workspace(n)
        else:
            ws, need = workspace, self.workspace_bytes(n)
            if ws.dtype != torch.uint8 or ws.numel() < need:
                raise ValueError(f"FrameScaler: workspace of {need} uint8 elements needed, {ws.numel()} {ws.dtype} given")
        (xb, xc, xk), (yb, yc, yk) = self.x_tables, self.y_tables
        _lib.launch("ir2rgb_frame_scale_u8", frames_u8, frames_u8, out, ws, need, xb, xc, xk, yb, yc, yk, n, *self._geom,
                    int(self.flip), int(normalised))
        return out
