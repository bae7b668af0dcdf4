"""Frame-by-frame video translation with a trained generator: the reference's test-time path.

    Vid2VidGenerator.inference / generate_frame_infer / generate_first_frame     models/generator.py:184-235
    the loop that drives it (change_seq -> fake_B_prev = None)                    test_vid2vid.py:36-60
    ToTensor + Normalize(0.5, 0.5), build_pyr, util.tensor2im                     data/transform.py:82-85,
                                                                                  base_model.py:64-82, util/util.py:45-67

The generator forward IS the training forward under ``no_grad`` (ir2rgb_amd.networks on the HIP kernels): neither
test_vid2vid.py nor prepare_models ever calls ``.eval()``, so the reference normalises every frame with that frame's
batch statistics.  What this module adds is what a frame loop needs around that forward:

* the recurrence state on the device -- per spatial scale one history of the last tG input frames ``[tG][C][h][w]`` and one
  of the last tG-1 generated frames ``[tG-1][3][h][w]``, fp32, oldest first.  Viewed as ``[1, T*C, h, w]`` a history is the
  generator's channel-stacked operand, so nothing is concatenated or re-pooled per frame;
* the 8-bit image boundary as two HIP kernels (csrc/frame_io.hip): ``ir2rgb_frame_push_u8`` normalises a uint8 HWC frame
  into the newest slot of the input history and pools it into the half-resolution one, ``ir2rgb_frame_finish_u8`` files a
  generated frame into its history and writes the uint8 HWC image; both shift their history in place;
* one HIP-graph replay per frame: after two eager steps at a shape, every step that is not the first of its sequence is
  one captured graph (push, coarser pyramid levels, every scale's generator with its two branch streams, finish per
  scale) working on the static histories.  The first step of a sequence stays eager (``use_raw_only`` and the history
  initialisation differ there); ``reset()`` keeps the graph;
* camera-size frames: with ``source_size`` (or a ``FrameScaler``) uint8 frames of the camera's size are scaled, cropped and
  flipped on the device exactly as the reference's loader does with Pillow (ir2rgb_amd.transform, csrc/frame_scale.hip)
  into the staging buffer ``ir2rgb_frame_push_u8`` reads; the two launches are part of the captured step;
* raw thermal frames: with ``agc`` (an ``ir2rgb_amd.thermal.ThermalAGC``) 16-bit counts are tone-mapped on the device
  (csrc/thermal_agc.hip) into the staging buffer the scaler or ``ir2rgb_frame_push_u8`` reads; its three launches are part
  of the captured step too, and its damped histogram and sequence-start flag live on the device, so a replay needs no
  host argument.

There is no CPU path: a CPU device raises, as everywhere in this package.
"""
import os

import torch

from . import _lib, autograd, checkpoint, layers, networks

__all__ = ["VideoTranslator", "SequenceState", "normalise_u8", "to_u8", "frame_push", "frame_finish"]


def normalise_u8(frame_u8):
    """uint8 [H,W,C] -> fp32 [C,H,W] by transforms.ToTensor + Normalize(0.5, 0.5) in torch's operation order (the
    arithmetic ir2rgb_frame_push_u8 implements; plain torch, any device)."""
    return frame_u8.permute(2, 0, 1).float().div(255).sub(0.5).div(0.5)


def to_u8(image):
    """fp32 [3,H,W] -> uint8 [H,W,3] by util.tensor2im's expression ``clip((x + 1) / 2 * 255, 0, 255).astype(uint8)``
    evaluated in fp32 in that order (the arithmetic ir2rgb_frame_finish_u8 implements; plain torch, any device)."""
    return image.permute(1, 2, 0).float().add(1).div(2).mul(255).clamp(0, 255).to(torch.uint8)


def frame_push(frame, hist0, hist1=None):
    """ir2rgb_frame_push_u8: ``frame`` uint8 [H,W,C] or fp32 [C,H,W] -> newest slot of ``hist0`` [T,C,H,W] (older slots
    move down) and its 3x3 stride-2 average into ``hist1`` [T,C,(H-1)//2+1,(W-1)//2+1] (None: one level only)."""
    _lib.require_device(frame, hist0, hist1)
    T, C, H, W = hist0.shape
    f32 = frame.dtype == torch.float32
    if hist0.dtype != torch.float32 or (hist1 is not None and hist1.dtype != torch.float32):
        raise TypeError("frame_push: histories are fp32")
    if not f32 and frame.dtype != torch.uint8:
        raise TypeError(f"frame_push: uint8 [H,W,C] or fp32 [C,H,W] frame expected, got {frame.dtype}")
    if tuple(frame.shape) != ((C, H, W) if f32 else (H, W, C)):
        raise ValueError(f"frame_push: frame {tuple(frame.shape)} does not fit the history {tuple(hist0.shape)}")
    if hist1 is not None and tuple(hist1.shape) != (T, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1):
        raise ValueError(f"frame_push: half-resolution history {tuple(hist1.shape)} does not fit {tuple(hist0.shape)}")
    _lib.launch("ir2rgb_frame_push_u8", hist0, frame, hist0, hist1, T, C, H, W, int(f32))


def frame_finish(x, hist, img_u8=None):
    """ir2rgb_frame_finish_u8: ``x`` fp32 [3,h,w] (or [1,3,h,w]) -> newest slot of ``hist`` [T,3,h,w] (older slots move
    down) and, when given, the uint8 [h,w,3] image."""
    _lib.require_device(x, hist, img_u8)
    T, c, h, w = hist.shape
    if x.dtype != torch.float32 or hist.dtype != torch.float32 or (img_u8 is not None and img_u8.dtype != torch.uint8):
        raise TypeError("frame_finish: fp32 frame and history, uint8 image expected")
    if c != 3 or x.numel() != 3 * h * w or tuple(x.shape[-3:]) != (3, h, w):
        raise ValueError(f"frame_finish: frame {tuple(x.shape)} does not fit the history {tuple(hist.shape)}")
    if img_u8 is not None and tuple(img_u8.shape) != (h, w, 3):
        raise ValueError(f"frame_finish: image {tuple(img_u8.shape)} is not [{h},{w},3]")
    _lib.launch("ir2rgb_frame_finish_u8", hist, x, hist, img_u8, T, h, w)


class SequenceState:
    """Frame counting of one sequence (host arithmetic only): how many input frames were pushed and whether a frame has
    been generated yet.  ``push()`` -> True when the frame just counted completes a window of tG input frames, i.e. a
    frame is to be generated; the first tG-1 frames of a sequence only fill the input history."""

    def __init__(self, tG):
        self.tG = int(tG)
        self.reset()

    def reset(self):
        self.n_pushed = 0           # input frames of this sequence so far
        self.started = False        # a frame of this sequence was generated (or a history was loaded)

    @property
    def warming(self):
        """True while the next frame still only fills the input history."""
        return self.n_pushed < self.tG - 1

    def push(self):
        self.n_pushed += 1
        return self.n_pushed >= self.tG

    def output_frame(self, k):
        """Index of the input frame whose translation is output ``k`` of the sequence: the first tG-1 frames produce
        none, so a ground-truth track is read at ``output_frame(k)``."""
        return self.tG - 1 + int(k)

    def begin_step(self):
        """-> is_first_frame of the step that starts now (generator.py:187)."""
        first, self.started = not self.started, True
        return first


def _defaults():
    from .vid2vid import DEFAULTS
    return dict(DEFAULTS)


class VideoTranslator:
    """Translates a video frame by frame (generator.py:184-235 statement for statement: scales coarse to fine, ``fake_B_feat``
    / ``flow_feat`` handed from scale to scale, ``use_raw_only = no_first_img and is_first_frame``, each scale's history
    updated after its forward).

        tr = VideoTranslator(device, height, width, netG=trainer.netG)       # or checkpoint_dir=..., which_epoch=...
        tr.reset()                                                           # a new sequence (test_vid2vid.py:39-40)
        rgb = tr.push(ir_u8)                  # uint8 [H,W,C] -> uint8 [H,W,3] device tensor; None for the first tG-1 frames
        for rgb in tr.translate(frames): ...
        paths = tr.save(frames, out_dir)      # the same frames as JPEG files, encoded on the device

    ``**opt`` takes the option names and defaults of ``Vid2VidTrainer`` (``n_scales_spatial``, ``first_layer_gen_filters``
    (alias ``ngf``), ``n_input_gen_frames``, ``no_flow``, ``compute_dtype`` ...).  ``netG``: a trainer's generator list, used
    as it is (shared parameters, nothing copied); otherwise the generators are built and ``checkpoint_dir`` loads
    ``{which_epoch}_net_G{s}.pth`` through ir2rgb_amd.checkpoint.  ``weights="ema"`` loads ``{which_epoch}_net_G{s}_ema.pth``
    instead -- the moving average of the generators' parameters a trainer with ``ema_decay`` saves (a missing file raises
    ``FileNotFoundError``); with ``netG`` pass ``trainer.ema_generators()``, and ``weights`` only names what they are.

    ``first_frame``: ``"zeros"`` is the reference's ``no_first_img`` (the model also generates the first frame from a zero
    history, raw image only); ``"real"`` is ``use_real_img`` (the first tG-1 RGB frames are given: ``real_rgb_u8`` of
    ``push`` or ``input_B`` of ``inference``).  The reference's third mode, ``use_single_G``, and ``fg`` are not built.

    ``norm_stats``: ``"batch"`` (default) is what the reference does -- the generators stay in training mode, every frame is
    normalised with its own batch statistics, AND THE RUNNING STATISTICS KEEP ADVANCING with every translated frame, as
    they do in the reference (its modules are never put into eval mode).  ``"running"`` puts the generators into
    ``.eval()``: the frozen-statistics kernels, nothing advances.  Either mode is set on the modules handed in.

    ``source_size=(Hs, Ws)``: uint8 frames of that size (``push``, ``translate``, ``evaluate`` and their ``real_rgb`` /
    ``targets``) are first brought to the network's size by ``ir2rgb_amd.transform.FrameScaler`` -- Pillow's bicubic
    ``resize`` to ``(height, width)``, or, with ``scale_opt`` (the reference's ``dataset_scale`` / ``dataset_crop`` /
    ``load_size`` / ``fine_size`` / ``is_train`` / ``flip`` options, drawn once here, ``scale_rng`` as in
    ``transform.img_params``), the scale, crop and flip the reference's loader would apply; ``scaler=`` hands in a
    ``FrameScaler`` built elsewhere (the translator works on a ``clone()`` of it: same tables, a workspace of its own).  Either way its result size must be ``(height, width)``.  Frames that already have the
    network's size, and every fp32 frame, are taken as before.

    ``agc``: an ``ir2rgb_amd.thermal.ThermalAGC`` for raw thermal input (the translator works on a ``clone()`` of it: same
    options, state and workspace of its own).  ``push``, ``translate``, ``evaluate`` and ``save`` then also take uint16 or
    int16 (reinterpreted as unsigned) ``[Hs,Ws]`` frames of the camera's counts, which are tone-mapped to 8 bits on the
    device before anything else happens to them.  The AGC's size is the scaler's ``src_hw`` when there is a scaler, else
    ``(height, width)``; its ``channels`` is ``input_nc``.  ``reset()`` also starts the AGC's sequence anew.  Without
    ``agc`` nothing is allocated or launched for it and a 16-bit frame is the ``TypeError`` it always was.

    Nothing requires grad and no parameter or packed weight is written.  Returned tensors are the caller's own (copies of
    the static buffers the graph works on)."""

    def __init__(self, device, height, width, netG=None, checkpoint_dir=None, which_epoch="latest", first_frame="zeros",
                 norm_stats="batch", use_graph=True, source_size=None, scaler=None, scale_opt=None, scale_rng=None,
                 weights="raw", agc=None, **opt):
        device = torch.device(device)
        if weights not in ("raw", "ema"):
            raise ValueError(f"weights: 'raw' (the last step's parameters) or 'ema' (their moving average), got {weights!r}")
        if device.type != "cuda":
            raise ValueError("VideoTranslator runs on an AMD GPU only (ir2rgb_amd has no CPU fallback)")
        o = _defaults()
        if "ngf" in opt:
            opt["first_layer_gen_filters"] = opt.pop("ngf")
        unknown = sorted(set(opt) - set(o) - {"use_single_G"})
        if unknown:
            raise TypeError(f"VideoTranslator: unknown options {unknown}")
        o.update(opt)
        if o["fg"]:
            raise NotImplementedError("foreground model (fg=True) is a dead branch for IR->RGB")
        if o.get("use_single_G"):
            raise NotImplementedError("first frame from a single-image generator (use_single_G) is a dead branch for IR->RGB")
        if first_frame not in ("zeros", "real"):
            raise ValueError("first_frame: 'zeros' (no_first_img) or 'real' (use_real_img)")
        if norm_stats not in ("batch", "running"):
            raise ValueError("norm_stats: 'batch' (the reference's behaviour) or 'running'")
        if o["output_nc"] != 3 or o["input_nc"] not in (1, 3):
            raise ValueError("VideoTranslator: input_nc in {1, 3} and output_nc == 3 (the uint8 image boundary)")
        self.opt, self.device = o, device
        self.H, self.W = int(height), int(width)
        self.tG, self.n_scales = int(o["n_input_gen_frames"]), int(o["n_scales_spatial"])
        if self.tG < 2:
            raise ValueError("n_input_gen_frames >= 2 (the generators take at least one previous frame)")
        self.first_frame, self.norm_stats, self.use_graph = first_frame, norm_stats, bool(use_graph)
        if netG is None:
            netG = self._build_generators(o)
            if checkpoint_dir is not None:
                for s, g in enumerate(netG):
                    label = f"G{s}_ema" if weights == "ema" else f"G{s}"
                    if weights == "ema" and not os.path.isfile(checkpoint.network_path(checkpoint_dir, label, which_epoch)):
                        raise FileNotFoundError(f"weights='ema': {checkpoint.network_path(checkpoint_dir, label, which_epoch)} is "
                                                "missing (written by save_trainer for a trainer with ema_decay)")
                    checkpoint.load_network(g, label, which_epoch, checkpoint_dir)
        elif checkpoint_dir is not None:
            raise ValueError("VideoTranslator: give netG or checkpoint_dir, not both")
        if len(netG) != self.n_scales:
            raise ValueError(f"VideoTranslator: {len(netG)} generators for n_scales_spatial={self.n_scales}")
        self.netG = list(netG)
        for g in self.netG:
            g.to(device)
            g.compute_dtype = o["compute_dtype"]
            g.train(norm_stats == "batch")
        self.seq = SequenceState(self.tG)
        self._jpeg = (None, None)       # (options, JpegEncoder) of the last save()
        self.scaler = self.scaler_rgb = None
        if scaler is not None or source_size is not None:
            self._set_scaler(scaler, source_size, scale_opt, scale_rng)
        elif scale_opt is not None:
            raise ValueError("VideoTranslator: scale_opt needs source_size")
        self.agc = None
        if agc is not None:
            self._set_agc(agc)
        self._alloc()

    def _set_scaler(self, scaler, source_size, scale_opt, scale_rng):
        from .transform import FrameScaler
        C = self.opt["input_nc"]
        if scaler is None:
            src_hw = (int(source_size[0]), int(source_size[1]))
            if scale_opt is not None:
                scaler = FrameScaler.from_options(self.device, src_hw, C, rng=scale_rng, **scale_opt)
            else:
                scaler = FrameScaler(self.device, src_hw, C, new_size=(self.W, self.H))
        elif scale_opt is not None or (source_size is not None and tuple(source_size) != scaler.src_hw):
            raise ValueError("VideoTranslator: give scaler, or source_size with scale_opt, not both")
        if scaler.channels != C or scaler.device != self.device:
            raise ValueError(f"VideoTranslator: the scaler takes {scaler.channels}-channel frames on {scaler.device}, "
                             f"input_nc={C} on {self.device} needed")
        if scaler.out_hw != (self.H, self.W):
            raise ValueError(f"VideoTranslator: the scaler's result is {scaler.out_hw}, the network takes {(self.H, self.W)}")
        # private copies (the tables are shared, the workspaces are not): the captured step holds the address of its
        # scaler's workspace, and nothing the caller does with the scaler handed in may touch that buffer
        self.scaler = scaler.clone()
        self.scaler_rgb = self.scaler if C == 3 else scaler.with_channels(3)

    def _set_agc(self, agc):
        from .thermal import ThermalAGC
        if not isinstance(agc, ThermalAGC):
            raise TypeError(f"VideoTranslator: agc is an ir2rgb_amd.thermal.ThermalAGC, got {type(agc)}")
        hw = self.scaler.src_hw if self.scaler is not None else (self.H, self.W)
        if agc.hw != hw or agc.channels != self.opt["input_nc"] or agc.device != self.device:
            raise ValueError(f"VideoTranslator: the AGC gives {agc.channels}-channel frames of {agc.hw} on {agc.device}, "
                             f"{self.opt['input_nc']}-channel frames of {hw} on {self.device} needed")
        # a private copy, as with the scaler: the captured step holds the addresses of its state and workspace
        self.agc = agc.clone()

    @staticmethod
    def _build_generators(o):
        tG = o["n_input_gen_frames"]
        g_in, g_prev = o["input_nc"] * tG, (tG - 1) * o["output_nc"]
        kw = {k: o[k] for k in ("gen_blocks", "n_local_enhancers", "feat_num", "n_blocks_local", "fg", "no_flow")}
        gs = [networks.build_generator_module(g_in, o["output_nc"], g_prev, o["first_layer_gen_filters"], o["gen_network"],
                                              o["gen_ds_layers"], o["norm"], 0, **kw)]
        for s in range(1, o["n_scales_spatial"]):
            gs.append(networks.build_generator_module(g_in, o["output_nc"], g_prev, o["first_layer_gen_filters"] // 2 ** s,
                                                      o["gen_network"] + "-local", o["gen_ds_layers"], o["norm"], s, **kw))
        return gs

    def _alloc(self):
        """The static buffers: histories per pyramid level (index 0 = full resolution, as ``build_pyr`` orders them), the
        staging buffers a replayed step reads its frame from, and the uint8 result."""
        dev, C = self.device, self.opt["input_nc"]
        sizes = [(self.H, self.W)]
        for _ in range(1, self.n_scales):
            h, w = sizes[-1]
            sizes.append(((h - 1) // 2 + 1, (w - 1) // 2 + 1))
        self.sizes = sizes
        self.hist_A = [torch.zeros((self.tG, C, h, w), dtype=torch.float32, device=dev) for h, w in sizes]
        self.hist_B = [torch.zeros((self.tG - 1, 3, h, w), dtype=torch.float32, device=dev) for h, w in sizes]
        self.stage = {"u8": torch.zeros((self.H, self.W, C), dtype=torch.uint8, device=dev),
                      "f32": torch.zeros((C, self.H, self.W), dtype=torch.float32, device=dev)}
        if self.scaler is not None:     # a camera-size frame waits here; the step scales it into stage["u8"]
            self.stage["cam"] = torch.zeros((*self.scaler.src_hw, C), dtype=torch.uint8, device=dev)
        if self.agc is not None:        # raw counts wait here; the step tone-maps them into stage["cam"] or stage["u8"]
            self.stage["raw"] = torch.zeros(self.agc.hw, dtype=torch.int16, device=dev)
        self.image = torch.zeros((self.H, self.W, 3), dtype=torch.uint8, device=dev)
        self._graphs = {}               # staging kind -> CUDAGraph of one non-first step
        self._eager_steps = 0

    # ------------------------------------------------------------------ sequence state
    def reset(self):
        """A new sequence (test_vid2vid.py:39-40: ``model.fake_B_prev = None``).  Captured graphs are kept."""
        self.seq.reset()
        for h in self.hist_B:           # generate_first_frame, no_first_img: a zero history (generator.py:219-220)
            h.zero_()
        if self.agc is not None:
            self.agc.reset()

    def set_history(self, frames_per_scale):
        """Replace the generated-frame history: ``frames_per_scale[i]`` fp32 [tG-1,3,h_i,w_i], index 0 = full resolution,
        oldest frame first (``fake_B_prev`` of generator.py:189).  The next frame is then not a first frame (restart from a
        known state, teacher forcing)."""
        if len(frames_per_scale) != self.n_scales:
            raise ValueError(f"set_history: {self.n_scales} scales expected")
        for dst, src in zip(self.hist_B, frames_per_scale):
            src = torch.as_tensor(src)
            if tuple(src.shape) != tuple(dst.shape):
                raise ValueError(f"set_history: {tuple(src.shape)} given where {tuple(dst.shape)} is kept")
            dst.copy_(src)
        self.seq.started = True

    def history(self):
        """The generated-frame histories (copies), index 0 = full resolution."""
        return [h.clone() for h in self.hist_B]

    # ------------------------------------------------------------------ frames in
    def _push_levels(self, frame, hists):
        """One frame into every level of a pyramid of histories: the first two levels in one launch, coarser ones by
        ir2rgb_avgpool3s2 of the level above (base_model.py:78-81)."""
        frame_push(frame, hists[0], hists[1] if len(hists) > 1 else None)
        for i in range(2, len(hists)):
            h = hists[i]
            for k in range(h.shape[0] - 1):
                h[k].copy_(h[k + 1])
            h[-1].copy_(autograd.avg_pool3s2(hists[i - 1][-1]))

    def _as_frame(self, frame, channels, what):
        frame = torch.as_tensor(frame)
        if frame.dtype == torch.uint8:
            if frame.dim() == 2:
                frame = frame.unsqueeze(-1)
            want = (self.H, self.W, channels)
            if self.scaler is not None and tuple(frame.shape) == (*self.scaler.src_hw, channels):
                want = tuple(frame.shape)                   # camera size: scaled on the device before it is used
        elif frame.dtype == torch.float32:
            want = (channels, self.H, self.W)
        elif self.agc is not None and what == "push" and frame.dtype in (torch.uint16, torch.int16):
            frame = frame.view(torch.int16)                 # the camera's counts: the same bits, a dtype torch can copy
            want = self.agc.hw
        else:
            raise TypeError(f"{what}: uint8 [H,W,C] or normalised fp32 [C,H,W] expected, got {frame.dtype}")
        if tuple(frame.shape) != want:
            raise ValueError(f"{what}: shape {tuple(frame.shape)} given, {want} expected")
        return frame.to(self.device).contiguous()

    def _camera_size(self, frame):
        return self.scaler is not None and frame.dtype == torch.uint8 and tuple(frame.shape[:2]) == self.scaler.src_hw

    def _tone_map(self, raw):
        """Raw counts -> the uint8 staging buffer of their size (``stage["cam"]`` with a scaler, else ``stage["u8"]``)."""
        return self.agc(raw, out=self.stage["cam" if self.scaler is not None else "u8"])

    def _rgb_frame(self, frame, what):
        """An RGB frame (first real frames, targets) at the network's size: camera-size uint8 frames are scaled."""
        frame = self._as_frame(frame, 3, what)
        return self.scaler_rgb(frame) if self._camera_size(frame) else frame

    def push(self, ir_u8, real_rgb_u8=None):
        """One input frame (uint8 [H,W,C], or [Hs,Ws,C] with ``source_size``; a normalised fp32 [C,H,W] tensor is taken
        too; with ``agc`` also the camera's 16-bit counts, uint16 or int16 [Hs,Ws]).  Returns the translated frame as a
        uint8 [H,W,3] device tensor, or None while fewer than tG input frames have been pushed.  With ``first_frame="real"`` the first tG-1 calls of a sequence also take that frame's real RGB image."""
        with torch.no_grad():
            frame = self._as_frame(ir_u8, self.opt["input_nc"], "push")
            warming = self.seq.warming
            if self.first_frame == "real" and warming and not self.seq.started:
                if real_rgb_u8 is None:
                    raise ValueError("first_frame='real': the first tG-1 frames of a sequence need real_rgb_u8")
                self._push_levels(self._rgb_frame(real_rgb_u8, "push(real_rgb_u8)"), self.hist_B)
            raw = frame.dtype == torch.int16
            if not self.seq.push():
                if raw:
                    frame = self._tone_map(frame)
                camera = self._camera_size(frame)
                self._push_levels(self.scaler(frame, out=self.stage["u8"]) if camera else frame, self.hist_A)
                return None
            camera = self._camera_size(frame)
            kind = "raw" if raw else ("cam" if camera else ("u8" if frame.dtype == torch.uint8 else "f32"))
            self.stage[kind].copy_(frame)
            self._step(kind)
            return self.image.clone()

    def translate(self, frames, real_rgb=None):
        """Generator over the translated frames of one sequence (``reset()`` first): ``frames`` any iterable of input
        frames, ``real_rgb`` the first tG-1 real RGB frames when ``first_frame="real"``."""
        self.reset()
        real_rgb = list(real_rgb) if real_rgb is not None else []
        for i, f in enumerate(frames):
            out = self.push(f, real_rgb[i] if i < len(real_rgb) else None)
            if out is not None:
                yield out

    def save(self, frames, out_dir, real_rgb=None, pattern="%06d.jpg", **jpeg_options):
        """``translate(frames, real_rgb)`` written to ``out_dir`` as one JPEG file per output frame (what the reference's
        test script does with ``save_images``): output ``k`` goes to ``pattern % k``.  -> the list of paths.

        The files are encoded on the device (``ir2rgb_amd.jpeg.JpegEncoder``; ``jpeg_options``: ``quality``,
        ``subsampling``, ``restart_rows``, Pillow's defaults otherwise) and are the bytes Pillow writes for the same frame
        and options.  Frame ``k`` is submitted to the encoder before file ``k - 1`` is collected and written, so the device
        encodes (and translates on) while the host writes.  The encoder's launches follow the step on the current stream;
        they are not part of the captured graph."""
        from .jpeg import JpegEncoder
        key = tuple(sorted(jpeg_options.items()))
        if self._jpeg[0] != key:
            self._jpeg = (key, JpegEncoder(self.device, self.H, self.W, channels=3, **jpeg_options))
        enc = self._jpeg[1]
        os.makedirs(out_dir, exist_ok=True)
        paths = []

        def write_oldest():
            data, = enc.collect()
            paths.append(os.path.join(out_dir, pattern % len(paths)))
            with open(paths[-1], "wb") as f:
                f.write(data)

        for k, out in enumerate(self.translate(frames, real_rgb)):
            enc.submit(out)
            if k:
                write_oldest()
        if enc.in_flight:
            write_oldest()
        return paths

    def evaluate(self, frames, targets, real_rgb=None, data_range="reference", temporal=None, colour=False):
        """``translate(frames, real_rgb)`` scored against a ground-truth RGB track (reference scripts/ssim_metric.py):
        output ``k`` is compared with ``targets[tG-1+k]`` -- ``targets`` is indexed like ``frames``, uint8 [H,W,3] each
        (camera-size ones are scaled like the frames), moved to the device if needed.
        -> ``ir2rgb_amd.metrics.VideoScore``; its ``result()`` is the only host
        synchronisation.  The scores are enqueued on the current stream after each step; the captured graph is the one
        ``translate`` replays.  ``data_range``: see ``ir2rgb_amd.metrics.video_metrics``.

        ``temporal``: a callable ``(cur, prev) -> (flow, conf)`` on normalised fp32 [n,3,H,W] frames -- an
        ``ir2rgb_amd.flownet.FlowNet`` or any stand-in.  With it every output ``k >= 1`` is also scored for flicker: the flow
        of the scaled targets, ``temporal(norm(T_k), norm(T_k-1))`` (the trainer's ``flowNet(real_B[:, 1:], real_B[:, :-1])``),
        gives ``warp_error(P_k-1, P_k, flow, conf)`` for the outputs and ``warp_error(T_k-1, T_k, flow, conf)`` for the
        targets as the baseline (``VideoScore.add_pair``; ``result()`` then has ``warp_l1``, ``warp_mse``, ``truth_warp_l1``,
        ``truth_warp_mse``, ``coverage``, ``pairs`` and ``per_pair``).  All of it is enqueued on the current stream after
        the step; None (default) scores frame by frame only.

        ``colour``: with True every output is also scored in colour against its target (``colour_metrics``: RGB PSNR and
        the CIELAB error, which the gray-only scores cannot see; ``result()`` then has ``mse``, ``psnr``, ``delta_e``,
        ``delta_l``, ``delta_c`` and ``per_frame_colour``).  False (default) launches and allocates nothing more."""
        from .metrics import VideoScore
        if not hasattr(targets, "__getitem__"):
            targets = list(targets)
        if temporal is not None and not callable(temporal):
            raise TypeError(f"evaluate: temporal is a callable (cur, prev) -> (flow, conf), got {type(temporal)}")
        score = VideoScore(data_range, colour)
        prev = None                                                     # (output, target) of the step before
        for k, out in enumerate(self.translate(frames, real_rgb)):
            i = self.seq.output_frame(k)
            if i >= len(targets):
                raise ValueError(f"evaluate: output {k} is scored against targets[{i}], {len(targets)} targets given")
            target = self._rgb_frame(targets[i], "evaluate(targets)")
            score.add(target, out)
            if temporal is not None:
                if prev is not None:
                    with torch.no_grad():
                        flow, conf = temporal(normalise_u8(target).unsqueeze(0).contiguous(),
                                              normalise_u8(prev[1]).unsqueeze(0).contiguous())
                    score.add_pair(prev[0].unsqueeze(0), out.unsqueeze(0), prev[1].unsqueeze(0), target.unsqueeze(0),
                                   flow.float().contiguous(), conf.float().contiguous())
                prev = (out, target)
        return score

    def inference(self, input_A, input_B=None):
        """The reference-shaped call (generator.py:184-195): ``input_A`` fp32 [1,tG,C,H,W] normalised, ``input_B`` fp32
        [1,>=tG-1,3,H,W] or None -> (fake_B [3,H,W] fp32, real_A[0][0,-1]).  The whole window is taken as given on every
        call, as the reference does; ``input_B`` is read only at the first call of a sequence with ``first_frame="real"``."""
        with torch.no_grad():
            C = self.opt["input_nc"]
            if input_A.dim() != 5 or tuple(input_A.shape) != (1, self.tG, C, self.H, self.W) or input_A.dtype != torch.float32:
                raise ValueError(f"inference: input_A fp32 [1,{self.tG},{C},{self.H},{self.W}] expected, got {tuple(input_A.shape)}")
            A = input_A.to(self.device).contiguous()
            if not self.seq.started and self.first_frame == "real":
                if input_B is None or tuple(input_B.shape[2:]) != (3, self.H, self.W) or input_B.shape[1] < self.tG - 1:
                    raise ValueError("first_frame='real': inference needs input_B [1,>=tG-1,3,H,W] at the first frame")
                B = input_B.to(self.device).float().contiguous()
                for t in range(self.tG - 1):                         # generator.py:221-222: real_B[:, :tG-1]
                    self._push_levels(B[0, t], self.hist_B)
            for t in range(self.tG - 1):
                self._push_levels(A[0, t], self.hist_A)
            self.seq.n_pushed = max(self.seq.n_pushed + 1, self.tG)
            self.stage["f32"].copy_(A[0, -1])
            self._step("f32")
            return self.hist_B[0][-1].clone(), A[0, -1]

    # ------------------------------------------------------------------ one frame
    def _step_body(self, kind, first):
        """push + generate_frame_infer for every scale (generator.py:191-195, :197-215) on the static buffers."""
        if kind == "raw":
            self._tone_map(self.stage["raw"])
            kind = "cam" if self.scaler is not None else "u8"
        if kind == "cam":
            self.scaler(self.stage["cam"], out=self.stage["u8"])
            kind = "u8"
        self._push_levels(self.stage[kind], self.hist_A)
        use_raw_only = self.first_frame == "zeros" and first            # no_first_img and is_first_frame
        feat = flow_feat = None
        ns = self.n_scales
        for s in range(ns):                                              # coarse to fine
            si = ns - 1 - s
            h, w = self.sizes[si]
            out = self.netG[s](self.hist_A[si].view(1, -1, h, w), self.hist_B[si].view(1, -1, h, w), None, feat, flow_feat,
                               None, use_raw_only)
            fake_B, feat, flow_feat = out[0], out[4], out[5]
            frame_finish(fake_B.float().contiguous(), self.hist_B[si], self.image if si == 0 else None)

    def _step(self, kind):
        first = self.seq.begin_step()
        if first or not self.use_graph or self._eager_steps < 2:
            self._step_body(kind, first)
            self._eager_steps += 1
            return
        g = self._graphs.get(kind)
        if g is None:
            # warm: packed weights, descriptor caches and the allocator have seen this shape twice (the discipline of
            # GraphedForward / FlowNet).  Capturing records the step without running it; the replay below runs it.
            import torch.distributed as dist
            layers.flush_bn_counters()
            torch.cuda.synchronize(self.device)
            g = torch.cuda.CUDAGraph()
            mode = "thread_local" if dist.is_available() and dist.is_initialized() else "global"
            with torch.cuda.graph(g, capture_error_mode=mode), networks.branch_streams(True):
                self._step_body(kind, False)
                layers.flush_bn_counters()
            self._graphs[kind] = g
        g.replay()
