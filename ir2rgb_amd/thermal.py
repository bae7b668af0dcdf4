"""Raw thermal input: a camera's automatic gain control (AGC), 16-bit counts -> 8-bit frames, on the device.

KAIST ships its ``lwir`` track tone-mapped to 8 bits; a microbolometer core and every radiometric recording deliver 14-16
bit counts of which a scene occupies a few hundred to a few thousand levels.  ``ThermalAGC`` (csrc/thermal_agc.hip) is
the tone mapping a camera does -- plateau histogram equalisation, or a percentile window -- on a histogram that is
damped over time, so the 8-bit frames the recurrent generator sees do not flicker.  Everything is integer arithmetic,
so ``agc_reference`` below (numpy, int64) DEFINES it and the kernels are held to it at tolerance 0, the state included.

All values are integers, ``>>`` is an arithmetic shift (a floor).  Per frame ``x`` (uint16 [H,W], ``P = H W``), with
``a_q = round(damping 65536)`` clamped to 0..65535:

    h[v] = pixels equal to v                                       v = 0..65535
    g[v] = min(h[v], plateau)   (plateau)        g[v] = h[v]   (linear)
    S = g << 16                                  on the first frame of a sequence,
    S = S + ((((g << 16) - S) (65536 - a_q)) >> 16)               afterwards              (int64, Q16)
    C[v] = S[0] + ... + S[v],  T = C[65535]
    plateau:  v0, v1 = smallest, largest v with S[v] > 0;  c0 = C[v0];  D = T - c0
              lut[v] = (max(C[v] - c0, 0) 255 + D // 2) // D,  all 0 when D == 0;  levels = (v0, v1)
    linear:   lo = min{v : C[v] 10^6 > T tail_ppm},  hi = min{v : C[v] 10^6 >= T (10^6 - tail_ppm)},  Wd = hi - lo
              lut[v] = clamp(((v - lo) 255 + Wd // 2) // Wd, 0, 255),  all 0 when Wd == 0;  levels = (lo, hi)
    y[p, c] = lut[x[p]]

The step moves S toward ``g << 16`` and never past it: ``0 <= S <= max(S_prev, g << 16)``, ``sum S <= P 2^16``, and a
level with pixels on it never reaches 0, so ``T > 0`` always.  With ``P <= 2^26`` every product fits int64.
"""
import numpy as np

__all__ = ["ThermalAGC", "agc_reference", "agc_options"]

LEVELS = 65536
CHUNK = 16                      # frames per launch triple; longer inputs are walked in chunks against one workspace
MODES = {"plateau": 0, "linear": 1}


def agc_options(P, mode="plateau", plateau=None, damping=0.875, tail_ppm=10000, channels=3):
    """The options as the integers both implementations work on -> (mode index, plateau, a_q, tail_ppm, channels);
    anything out of range raises ValueError."""
    if mode not in MODES:
        raise ValueError(f"agc: mode 'plateau' or 'linear', got {mode!r}")
    P = int(P)
    if not 1 <= P <= 1 << 26:
        raise ValueError(f"agc: frames of 1 to 2^26 pixels, got {P}")
    plateau = max(1, P // 1024) if plateau is None else int(plateau)
    if not 1 <= plateau <= 0x7fffffff:
        raise ValueError(f"agc: plateau >= 1, got {plateau}")
    if not 0 <= damping < 1:
        raise ValueError(f"agc: damping in [0, 1), got {damping}")
    a_q = min(max(int(round(float(damping) * 65536)), 0), 65535)
    tail_ppm = int(tail_ppm)
    if not 0 <= tail_ppm < 500000:
        raise ValueError(f"agc: tail_ppm in [0, 500000), got {tail_ppm}")
    if int(channels) not in (1, 3):
        raise ValueError(f"agc: 1 or 3 channels, got {channels}")
    return MODES[mode], plateau, a_q, tail_ppm, int(channels)


def _as_counts(frames):
    """uint16 [N,H,W] from uint16 / int16 (reinterpreted as unsigned) [N,H,W] or [H,W] -> (array, had no N axis)."""
    frames = np.asarray(frames)
    if frames.dtype == np.int16:
        frames = frames.view(np.uint16)
    if frames.dtype != np.uint16:
        raise TypeError(f"agc: uint16 or int16 frames expected, got {frames.dtype}")
    if frames.ndim not in (2, 3) or frames.size == 0:
        raise ValueError(f"agc: frames [N,H,W] or [H,W] expected, got {frames.shape}")
    return (frames[None], True) if frames.ndim == 2 else (frames, False)


def agc_reference(frames, mode="plateau", plateau=None, damping=0.875, tail_ppm=10000, channels=3, state=None):
    """The definition (module docstring) in numpy: ``frames`` uint16 (or int16, reinterpreted) [N,H,W] or [H,W], the
    consecutive frames of one sequence -> ``(u8, levels, S)``: uint8 [N,H,W,channels] (no N axis for one [H,W] frame),
    int32 [N,2], and the state int64 [65536] behind the last frame.  ``state``: the ``S`` an earlier call returned, to go
    on with that sequence; None starts one."""
    x, single = _as_counts(frames)
    N, H, W = x.shape
    m, plateau, a_q, tail_ppm, channels = agc_options(H * W, mode, plateau, damping, tail_ppm, channels)
    S = None if state is None else np.array(state, dtype=np.int64)
    if S is not None and S.shape != (LEVELS,):
        raise ValueError(f"agc_reference: state int64 [{LEVELS}] expected, got {S.shape}")
    out = np.empty((N, H, W, channels), np.uint8)
    levels = np.empty((N, 2), np.int32)
    v = np.arange(LEVELS, dtype=np.int64)
    for n in range(N):
        h = np.bincount(x[n].ravel(), minlength=LEVELS).astype(np.int64)
        g = np.minimum(h, plateau) if m == 0 else h
        G = g << 16
        S = G if S is None else S + (((G - S) * (65536 - a_q)) >> 16)
        C = np.cumsum(S)
        T = int(C[-1])
        if m == 0:
            occupied = np.flatnonzero(S > 0)
            a, b = int(occupied[0]), int(occupied[-1])
            D = T - int(C[a])
            lut = (np.maximum(C - C[a], 0) * 255 + D // 2) // D if D else np.zeros(LEVELS, np.int64)
        else:
            a = int(np.argmax(C * 1000000 > T * tail_ppm))
            b = int(np.argmax(C * 1000000 >= T * (1000000 - tail_ppm)))
            Wd = b - a
            lut = np.clip(((v - a) * 255 + Wd // 2) // Wd, 0, 255) if Wd else np.zeros(LEVELS, np.int64)
        levels[n] = a, b
        out[n] = lut.astype(np.uint8)[x[n]][..., None]
    return (out[0] if single else out), levels, S


class ThermalAGC:
    """The camera's AGC on the device (csrc/thermal_agc.hip), equal to ``agc_reference`` bit for bit.

        agc = ThermalAGC("cuda:0", 512, 640, mode="plateau", plateau=None, damping=0.875, tail_ppm=10000, channels=3)
        u8 = agc(raw_u16)        # uint16 or int16 (reinterpreted as unsigned) [N,H,W] or [H,W], device or host
                                 # -> uint8 [N,H,W,C] ([H,W,C] for one [H,W] frame); the frames continue the sequence
        agc(raw_u16, out=buf)    # into a caller's contiguous uint8 buffer of that shape
        agc.levels               # int32 [N,2] device tensor of the last call: (v0, v1) or (lo, hi) per frame
        agc.state()              # int64 [65536] copy of S (synchronises)
        agc.reset()              # the next frame starts a sequence
        agc.clone()              # same options, own state and workspace

    ``plateau`` None is ``max(1, H W // 1024)``.  The damped histogram and the sequence-start flag live on the device: a
    call is three launches per 16 frames on the current stream, with no host synchronisation and no allocation when
    ``out`` is given and the frames are a contiguous device tensor of at most 16 frames -- so it can be captured in a
    HIP graph, and the replay is right for the first and for every later frame of a sequence.  Calls on one object
    share its state and workspace and belong on one stream."""

    def __init__(self, device, height, width, mode="plateau", plateau=None, damping=0.875, tail_ppm=10000, channels=3):
        import torch
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError("ThermalAGC runs on an AMD GPU only (ir2rgb_amd has no CPU fallback; agc_reference is the CPU oracle)")
        self.device, self.hw = device, (int(height), int(width))
        if min(self.hw) < 1:
            raise ValueError("ThermalAGC: sizes must be positive")
        self.mode, self.damping = mode, float(damping)
        self._mode, self.plateau, self.a_q, self.tail_ppm, self.channels = agc_options(
            self.hw[0] * self.hw[1], mode, plateau, damping, tail_ppm, channels)
        self._alloc()

    def _alloc(self):
        import torch
        from . import _lib
        dev = self.device
        self._ws_bytes = int(_lib.query("ir2rgb_thermal_agc_workspace_bytes", CHUNK, *self.hw))
        self._ws = torch.zeros(self._ws_bytes, dtype=torch.uint8, device=dev)       # zero between calls, never replaced
        self._state = torch.zeros(LEVELS + 1, dtype=torch.int64, device=dev)        # S and the sequence-start flag
        self._lut = torch.empty((CHUNK, LEVELS), dtype=torch.uint8, device=dev)
        self._levels = torch.zeros((CHUNK, 2), dtype=torch.int32, device=dev)
        self.levels = self._levels[:0]

    def reset(self):
        """A new sequence: the next frame initialises the histogram state (one memset of the flag word)."""
        self._state[LEVELS:].zero_()

    def clone(self):
        """The same options with a state (reset) and a workspace of its own."""
        import copy
        agc = copy.copy(self)
        agc._alloc()
        return agc

    def state(self):
        """int64 [65536] copy of S behind the calls enqueued so far (a device tensor; reading it synchronises)."""
        return self._state[:LEVELS].clone()

    def luts(self):
        """uint8 [n,65536]: the tables of the last (at most 16) frames processed (a copy)."""
        return self._lut[:min(max(self.levels.shape[0], 1), CHUNK)].clone()

    def _frames(self, raw):
        import torch
        raw = torch.as_tensor(raw)
        if raw.dtype == torch.uint16:
            raw = raw.view(torch.int16)             # uint16 has copies and views only; the kernels read the same bits
        if raw.dtype != torch.int16:
            raise TypeError(f"ThermalAGC: uint16 or int16 frames expected, got {raw.dtype}")
        if raw.dim() not in (2, 3) or tuple(raw.shape[-2:]) != self.hw:
            raise ValueError(f"ThermalAGC: frames {tuple(raw.shape)} given, [N,]{self.hw} expected")
        if raw.dim() == 3 and raw.shape[0] < 1:
            raise ValueError("ThermalAGC: an empty batch")
        return raw.to(self.device).contiguous()

    def __call__(self, raw, out=None):
        import torch
        from . import _lib
        x = self._frames(raw)
        single = x.dim() == 2
        n = 1 if single else x.shape[0]
        H, W = self.hw
        want = (H, W, self.channels) if single else (n, H, W, self.channels)
        if out is None:
            out = torch.empty(want, dtype=torch.uint8, device=self.device)
        else:
            _lib.require_device(out)
            if tuple(out.shape) != want or out.dtype != torch.uint8 or out.device != self.device:
                raise ValueError(f"ThermalAGC: out {tuple(out.shape)} {out.dtype} given, {want} torch.uint8 on {self.device} expected")
        levels = self._levels if n <= CHUNK else torch.empty((n, 2), dtype=torch.int32, device=self.device)
        xs, os_ = x.view(n, H * W), out.view(n, H * W * self.channels)
        for i in range(0, n, CHUNK):
            k = min(CHUNK, n - i)
            _lib.launch("ir2rgb_thermal_agc_u16", x, xs[i], os_[i], self._state, self._lut, levels[i:], self._ws,
                        self._ws_bytes, k, H, W, self.channels, self._mode, self.plateau, self.a_q, self.tail_ppm)
        self.levels = levels[:n]
        return out
