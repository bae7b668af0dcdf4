"""Training snapshots: what the reference shows of a run every ``display_freq`` sequences, composed on the device.

    util.save_all_tensors / tensor2im / tensor2flow          util/util.py:13-104
    Visualizer.display_current_results                       util/visualizer.py:38-90
    save_fake and the call                                   train_vid2vid.py:46, :131-136

The reference takes nine whole fp32 tensors to the host (a forced synchronisation and ~44 MB over PCIe at 512x1024),
converts them with numpy and cv2 and encodes JPEGs inside the loop.  Here one entry point of the kernel library
(csrc/visuals.hip) turns the tensors the trainer already holds into one uint8 ``[P, H, W, 3]`` stack; only those bytes are
copied out, asynchronously, and the files are written when the copy has long finished:

* ``panels(tensors, opt)``            the ordered (name, kind, tensor) list of ``save_all_tensors`` for ``label_nc == 0``
* ``compose(panel_list, ...)``        the launch: -> uint8 device tensor [P, H, W, 3] (GPU only)
* ``Snapshots``                        launch + pinned copy + event in ``take``, files and ``index.html`` one snapshot later
* ``to_u8_reference`` / ``flow_to_rgb_reference`` / ``hsv_bytes_to_rgb``   the same definitions on the CPU

What the reference pins and what it does not.  ``tensor2im`` (numpy only) and the panel list are pinned by the
reference's own code (tests/golden/visuals_*.npz).  ``tensor2flow`` goes through OpenCV's ``cartToPolar`` (an
approximation good to about 0.3 degrees), ``normalize`` and ``cvtColor``; the flow coding here is the HSV semantics those
calls document, evaluated exactly:

    mag = sqrt(u^2 + v^2),  ang = atan2(v, u) in [0, 2 pi)
    Hb  = trunc(ang * 90 / pi) mod 180                              (hsv[..., 0] = ang * 180 / pi / 2, 8-bit hue in [0, 180))
    Vb  = trunc((mag - min) * 255 / (max - min))                    (NORM_MINMAX to [0, 255]); 0 everywhere when max == min,
                                                                    0 for a NaN magnitude (min / max ignore NaN);  S = 255
    i = Hb // 30, r = Hb % 30, t = (2 Vb r + 30) // 60, q = (2 Vb (30 - r) + 30) // 60, p = 0
    (R, G, B) = (V,t,p) (q,V,p) (p,V,t) (p,q,V) (t,p,V) (V,p,q)[i]  (8-bit HSV -> RGB, round half up, integers only)
"""
import os

import numpy as np
import torch

from . import _lib
from . import streamcheck as SC

__all__ = ["IMAGE_NORM", "IMAGE_UNIT", "FLOW", "to_u8_reference", "flow_to_rgb_reference", "hsv_bytes_to_rgb", "panels",
           "compose", "Snapshots"]

IMAGE_NORM, IMAGE_UNIT, FLOW = _lib.PANEL_IMAGE_NORM, _lib.PANEL_IMAGE_UNIT, _lib.PANEL_FLOW
DECIDED_BAND = 1e-3      # a flow pixel is decided when both of its scaled values are farther than this from an integer


# ---------------------------------------------------------------------------------------------
# the definitions on the CPU
# ---------------------------------------------------------------------------------------------
def _last_frame(x):
    """tensor2im's indexing: [B,T,C,H,W] -> [0, -1], [B,C,H,W] -> [0]."""
    if x.dim() == 5:
        x = x[0, -1]
    if x.dim() == 4:
        x = x[0]
    if x.dim() != 3:
        raise ValueError(f"a [C,H,W], [B,C,H,W] or [B,T,C,H,W] tensor expected, got {tuple(x.shape)}")
    return x


_TO_INTEGER = np.trunc       # astype(uint8) of a value in [0, 255] truncates (tests plant np.rint here)


def to_u8_reference(x, normalize=True):
    """``util.tensor2im(x, normalize=normalize)`` (util/util.py:45-68) in numpy fp32: uint8 [H,W,3], or [H,W] for one
    channel.  NaN gives 0 (numpy leaves that cast undefined; the kernels define it)."""
    a = _last_frame(torch.as_tensor(x))[:3].detach().cpu().float().numpy()
    a = np.transpose(a, (1, 2, 0))
    a = (a + 1) / 2.0 * 255.0 if normalize else a * 255.0
    a = np.nan_to_num(np.clip(a, 0, 255), nan=0.0)
    if a.shape[2] == 1:
        a = a[:, :, 0]
    return _TO_INTEGER(a).astype(np.uint8)


def hsv_bytes_to_rgb(hb, vb):
    """8-bit HSV -> RGB at S = 255 with hue in [0, 180): integer arrays ``hb``, ``vb`` -> uint8 [..., 3]."""
    hb, vb = np.asarray(hb, dtype=np.int64) % 180, np.asarray(vb, dtype=np.int64)
    i, r = hb // 30, hb % 30
    t, q, p = (2 * vb * r + 30) // 60, (2 * vb * (30 - r) + 30) // 60, np.zeros_like(vb)
    table = [(vb, t, p), (q, vb, p), (p, vb, t), (p, q, vb), (t, p, vb), (vb, p, q)]
    out = np.zeros(hb.shape + (3,), dtype=np.uint8)
    for k, rgb in enumerate(table):
        for c in range(3):
            out[..., c] = np.where(i == k, rgb[c], out[..., c])
    return out


def flow_to_rgb_reference(flow):
    """The flow coding of the module docstring with its floats-to-bytes stage in fp64 from the fp32 inputs.
    -> (rgb uint8 [H,W,3], decided bool [H,W], hb int [H,W], vb int [H,W]).  A pixel is *decided* when ``ang * 90 / pi``
    and ``(mag - min) * 255 / (max - min)`` are both farther than 1e-3 from an integer, i.e. when no fp32 evaluation of the
    same formulas can land on another byte; a ``max == min`` panel is decided everywhere and is black."""
    f = _last_frame(torch.as_tensor(flow)).detach().cpu().float().numpy().astype(np.float64)
    if f.shape[0] != 2:
        raise ValueError(f"a flow has two channels, got {f.shape[0]}")
    u, v = f[0], f[1]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        mag = np.sqrt(u * u + v * v)
        ang = np.arctan2(v, u)
        ang = np.where(ang < 0, ang + 2 * np.pi, ang)
        h = np.nan_to_num(ang * 90 / np.pi, nan=0.0)
        hb = np.trunc(np.clip(h, 0, 180)).astype(np.int64) % 180
        finite = mag[~np.isnan(mag)]
        mn, mx = (finite.min(), finite.max()) if finite.size else (np.inf, -np.inf)
        if mx > mn:
            val = (mag - mn) * 255 / (mx - mn)
        else:
            val = np.zeros_like(mag)
        val = np.nan_to_num(np.clip(val, 0, 255), nan=0.0)
        vb = np.trunc(val).astype(np.int64)
    if mx > mn:
        decided = (np.abs(h - np.rint(h)) > DECIDED_BAND) & (np.abs(val - np.rint(val)) > DECIDED_BAND)
    else:
        decided = np.ones(mag.shape, dtype=bool)
    return hsv_bytes_to_rgb(hb, vb), decided, hb, vb


# ---------------------------------------------------------------------------------------------
# the panel list
# ---------------------------------------------------------------------------------------------
def _opt(opt, key):
    return opt[key] if hasattr(opt, "__getitem__") else getattr(opt, key)


def panels(tensors, opt, input_panel="reference"):
    """``util.save_all_tensors`` (util/util.py:13-41) for ``label_nc == 0``: the ordered ``(name, kind, tensor)`` list,
    every tensor the [C,H,W] view ``tensor2im`` / ``tensor2flow`` would convert (no copy).

    ``tensors``: a mapping with ``real_A, fake_B, fake_B_first, fake_B_raw, real_B, flow_ref, conf_ref`` and ``flow``,
    ``weight`` (None when the generator returned no flow: ``no_flow``).  ``opt``: ``input_nc``.  ``input_panel``:
    ``"reference"`` shows the normalised input un-denormalised as the reference does (negative values come out black);
    ``"normalised"`` shows it as an image."""
    if input_panel not in ("reference", "normalised"):
        raise ValueError("input_panel: 'reference' or 'normalised'")
    c = 3 if _opt(opt, "input_nc") >= 3 else 1
    t = tensors
    out = [("input_image", IMAGE_UNIT if input_panel == "reference" else IMAGE_NORM, t["real_A"][0, -1, :c]),
           ("fake_image", IMAGE_NORM, _last_frame(t["fake_B"])[:3]),
           ("fake_first_image", IMAGE_NORM, _last_frame(t["fake_B_first"])[:3]),
           ("fake_raw_image", IMAGE_NORM, _last_frame(t["fake_B_raw"])[:3]),
           ("real_image", IMAGE_NORM, _last_frame(t["real_B"])[:3]),
           ("flow_ref", FLOW, _last_frame(t["flow_ref"])),
           ("conf_ref", IMAGE_UNIT, _last_frame(t["conf_ref"])[:3])]
    if t.get("flow") is not None:
        out += [("flow", FLOW, _last_frame(t["flow"])), ("weight", IMAGE_UNIT, _last_frame(t["weight"])[:3])]
    return out


def trainer_tensors(trainer, fake_B_first):
    """The arguments of the reference's ``save_all_tensors`` call as the trainer holds them after a window."""
    real_A, real_B, flow_ref, conf_ref = trainer.last_inputs
    fake_B, fake_B_raw, flow, weight = trainer.last_outputs
    return dict(real_A=real_A, fake_B=fake_B, fake_B_first=fake_B_first, fake_B_raw=fake_B_raw, real_B=real_B,
                flow_ref=flow_ref, conf_ref=conf_ref, flow=flow, weight=weight)


def reference_images(panel_list):
    """name -> uint8 array of every panel by the CPU definitions ([H,W] for one channel, as the reference saves them)."""
    return {name: flow_to_rgb_reference(t)[0] if kind == FLOW else to_u8_reference(t, normalize=kind == IMAGE_NORM)
            for name, kind, t in panel_list}


# ---------------------------------------------------------------------------------------------
# the launch
# ---------------------------------------------------------------------------------------------
def workspace_elems(n_flow, H, W):
    return _lib.query("ir2rgb_visuals_workspace_bytes", n_flow, H, W) // 4


def compose(panel_list, out=None, workspace=None):
    """``[(name, kind, fp32 device tensor [C,H,W])]`` -> the uint8 device stack [P,H,W,3] (csrc/visuals.hip), on the
    current stream.  ``out`` / ``workspace``: preallocated buffers (``Snapshots`` keeps them per shape)."""
    if not panel_list:
        raise ValueError("compose: no panels")
    srcs = [t for _, _, t in panel_list]
    dev = _lib.require_device(*srcs, dtype=torch.float32)
    H, W = srcs[0].shape[-2:]
    for name, _, t in panel_list:
        if t.dim() != 3 or tuple(t.shape[-2:]) != (H, W):
            raise ValueError(f"compose: panel {name!r} is {tuple(t.shape)}, [C,{H},{W}] expected")
    n = len(panel_list)
    table = (_lib.Panel * n)()
    for q, (_, kind, t) in zip(table, panel_list):
        q.src, q.kind, q.channels = t.data_ptr(), int(kind), t.shape[0]
    n_flow = sum(1 for _, kind, _ in panel_list if kind == FLOW)
    if out is None:
        out = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)
    if workspace is None and n_flow:
        workspace = torch.empty(workspace_elems(n_flow, H, W), dtype=torch.float32, device=dev)
    if SC.ENABLED:
        for t in srcs:
            SC.consumed(t, "snapshot panel source")
    _lib.launch("ir2rgb_visuals_u8", srcs[0], table, n, H, W, workspace if n_flow else None, out)
    return out


# ---------------------------------------------------------------------------------------------
# snapshots of a training run
# ---------------------------------------------------------------------------------------------
class Snapshots:
    """The visualiser of a training run (``fit(..., snapshots=Snapshots(...))``).

    ``take`` queues the panel kernels and the copy of the 8-bit stack into one of two pinned host buffers on the current
    stream, records an event and returns: nothing waits for the GPU.  The snapshot is written to
    ``{out_dir}/images/epoch%.3d_%s.{fmt}`` (the reference's labels, visualizer.py:58-62; one-channel panels as mode L) at
    the start of the next ``take`` or in ``flush()``, after that event.  ``html``: ``{out_dir}/index.html`` lists every
    epoch, newest first, in the two rows of visualizer.py:84-89.  ``freq`` is the reference's ``display_freq``: ``fit``
    takes a snapshot after every sequence that brings ``total_steps`` to a multiple of it.

    ``encoder``: ``"host"`` (default) copies the raw stack out and lets Pillow compress it in ``write_pending``.
    ``"device"`` compresses the panels on the device (ir2rgb_amd.jpeg.JpegEncoder with Pillow's defaults: quality 75,
    4:2:0, mode L for one-channel panels, one restart marker per MCU row) inside ``take``; only the file sizes and then the
    compressed bytes are copied.  It needs ``fmt="jpg"``.  A decoder reads the same pixels from either file."""

    def __init__(self, device, out_dir, freq=100, fmt="jpg", html=True, input_panel="reference", encoder="host"):
        if freq < 1:
            raise ValueError("Snapshots: freq >= 1")
        if input_panel not in ("reference", "normalised"):
            raise ValueError("input_panel: 'reference' or 'normalised'")
        if encoder not in ("host", "device"):
            raise ValueError("encoder: 'host' (Pillow) or 'device' (csrc/jpeg.hip)")
        if encoder == "device" and fmt != "jpg":
            raise ValueError("Snapshots: encoder='device' writes JPEG files (fmt='jpg')")
        self.encoder = encoder
        self.device, self.out_dir, self.freq, self.fmt, self.html = torch.device(device), str(out_dir), int(freq), fmt, html
        self.input_panel = input_panel
        self.img_dir = os.path.join(self.out_dir, "images")
        self.count = 0                  # snapshots taken
        self.names = []                 # panel names of the newest snapshot written (index.html lists those)
        self._shape = None              # (P, H, W, number of flow panels) the buffers below were made for
        self._stack = self._workspace = None
        self._host = [None, None]
        self._pending = None            # (host buffer index, event, epoch, [(name, channels)])
        self._jpeg = None               # encoder="device": see _reserve_jpeg

    def due(self, total_steps):
        """train_vid2vid.py:46 with ``total_steps`` as it stands after the sequence."""
        return total_steps % self.freq == 0

    def _reserve(self, n, H, W, n_flow):
        if self._shape != (n, H, W, n_flow):
            self.flush()
            self._stack = torch.empty((n, H, W, 3), dtype=torch.uint8, device=self.device)
            self._workspace = torch.empty(max(workspace_elems(n_flow, H, W), 1), dtype=torch.float32, device=self.device)
            if self.encoder == "device":
                self._reserve_jpeg(n, H, W)
            else:
                self._host = [torch.empty((n, H, W, 3), dtype=torch.uint8, pin_memory=True) for _ in range(2)]
            self._shape = (n, H, W, n_flow)

    def _reserve_jpeg(self, n, H, W):
        """The device encoders (three-channel panels; channel 0 of the stack as mode L), one output row and one size per
        panel, and the pinned staging of the sizes and of one file."""
        from .jpeg import JpegEncoder
        enc = {3: JpegEncoder(self.device, H, W), 1: JpegEncoder(self.device, H, W, channels=3, subsampling="L")}
        cap = max(e.capacity for e in enc.values())
        self._jpeg = dict(enc=enc, out=torch.empty((n, cap), dtype=torch.uint8, device=self.device),
                          lengths=torch.empty(n, dtype=torch.int32, device=self.device),
                          workspace=torch.empty(max(e.workspace_bytes(1) for e in enc.values()), dtype=torch.uint8,
                                                device=self.device),
                          host_lengths=torch.empty(n, dtype=torch.int32, pin_memory=True),
                          host=torch.empty(cap, dtype=torch.uint8, pin_memory=True))

    def _encode_panels(self, plist):
        j = self._jpeg
        for i, (_, _, t) in enumerate(plist):
            j["enc"][1 if t.shape[0] == 1 else 3].encode_into(self._stack[i:i + 1], j["out"][i:i + 1], j["lengths"][i:i + 1],
                                                             j["workspace"])
        j["host_lengths"].copy_(j["lengths"], non_blocking=True)

    def take(self, trainer, epoch, fake_B_first):
        """Snapshot of the trainer's last window (``last_inputs`` / ``last_outputs``) and the sequence's first generated
        frame, on the current stream.  To be queued before the next ``train_window`` is issued: the reference flow and
        its confidence may be FlowNet2's static replay outputs."""
        self.write_pending()
        plist = panels(trainer_tensors(trainer, fake_B_first), trainer.opt, self.input_panel)
        H, W = plist[0][2].shape[-2:]
        self._reserve(len(plist), H, W, sum(1 for _, kind, _ in plist if kind == FLOW))
        with torch.cuda.device(self.device):
            compose(plist, self._stack, self._workspace)
            slot = self.count % 2
            if self.encoder == "device":
                self._encode_panels(plist)
            else:
                self._host[slot].copy_(self._stack, non_blocking=True)
            event = torch.cuda.Event()
            event.record()
            # FlowNet2's next replay overwrites flow_ref / conf_ref and may run AHEAD of this stream (it is ordered after
            # the previous window's backward passes only: Vid2VidTrainer.reference_flows): not before they are read
            side = trainer._flow_stream(plist[0][2])
            if side is not None:
                side.wait_event(event)
        self._pending = (slot, event, int(epoch), [(name, t.shape[0]) for name, _, t in plist])
        self.count += 1

    def write_pending(self):
        if self._pending is None:
            return
        slot, event, epoch, names = self._pending
        self._pending = None
        event.synchronize()
        if self.encoder == "device":
            self._write_files(epoch, names)
        else:
            write_images(self.img_dir, epoch, names, self._host[slot].numpy(), self.fmt)
        self.names = [name for name, _ in names]
        if self.html:
            write_index(self.out_dir, epoch, self.names, self.fmt)

    def _write_files(self, epoch, names):
        from .jpeg import fetch_file
        j = self._jpeg
        os.makedirs(self.img_dir, exist_ok=True)
        for i, (label, _) in enumerate(names):
            # (on a copy stream: not behind the windows queued since)
            data = fetch_file(j["out"][i], j["host_lengths"][i], j["host"], f"Snapshots: panel {label!r}")
            with open(os.path.join(self.img_dir, image_name(epoch, label, self.fmt)), "wb") as f:
                f.write(data)

    def flush(self):
        """Writes the snapshot that is still on its way (``fit`` calls this before it returns)."""
        self.write_pending()


def image_name(epoch, label, fmt):
    return "epoch%.3d_%s.%s" % (epoch, label, fmt)


def write_images(img_dir, epoch, names, stack, fmt="jpg"):
    """``stack`` uint8 [P,H,W,3], ``names`` [(label, channels)] -> one file per panel; one-channel panels as mode L."""
    from PIL import Image
    os.makedirs(img_dir, exist_ok=True)
    for (label, channels), img in zip(names, stack):
        im = Image.fromarray(np.ascontiguousarray(img[:, :, 0]), "L") if channels == 1 else Image.fromarray(np.ascontiguousarray(img), "RGB")
        im.save(os.path.join(img_dir, image_name(epoch, label, fmt)))


def write_index(out_dir, epoch, labels, fmt="jpg", width=256):
    """``{out_dir}/index.html``: epochs ``epoch`` .. 1, newest first, the panels of each in one row when there are fewer
    than six and in two rows of round(n / 2) and the rest otherwise (visualizer.py:66-90)."""
    rows = [labels] if len(labels) < 6 else [labels[:int(round(len(labels) / 2.0))], labels[int(round(len(labels) / 2.0)):]]
    cell = '<td><p><a href="images/%s"><img src="images/%s" style="width:%dpx"></a><br>%s</p></td>'
    parts = ["<!DOCTYPE html>", "<html><head><title>training snapshots</title></head><body>"]
    for n in range(epoch, 0, -1):
        parts.append("<h3>epoch [%d]</h3>" % n)
        for row in rows:
            cells = "".join(cell % (image_name(n, lb, fmt), image_name(n, lb, fmt), width, lb) for lb in row)
            parts.append('<table border="1" style="table-layout: fixed;"><tr>%s</tr></table>' % cells)
    parts.append("</body></html>")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "index.html"), "w") as f:
        f.write("\n".join(parts) + "\n")
