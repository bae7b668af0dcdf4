"""What the two halves of the baseline JPEG codec share on the host, each fact stated once (``jpeg``: frames -> files,
``jpeg_decode``: files -> frames).  csrc/jpeg_common.h is the device's side of the list: MODES is MODE_*, Geometry is
jpeg_grid, ZIGZAG is ZZ, the keys of F are F0_298 .. F3_072, descale is descale."""
import numpy as np

MODES = ("4:4:4", "4:2:0", "L", "4:2:2")            # the index is the ``mode`` of include/ir2rgb_hip.h: IR2RGB_JPEG_*
WRITTEN_MODES = MODES[:3]                           # 4:2:2 is read, not written
SAMPLING = {"4:4:4": (1, 1), "4:2:0": (2, 2), "L": (1, 1), "4:2:2": (2, 1)}

# natural (row-major) index of zigzag position k
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                   54, 47, 55, 62, 63], dtype=np.int64)

# jfdctint / jidctint: FIX(x) with CONST_BITS 13, keyed by x
F = dict(f0_298=2446, f0_390=3196, f0_541=4433, f0_765=6270, f0_899=7373, f1_175=9633, f1_501=12299, f1_847=15137, f1_961=16069,
         f2_053=16819, f2_562=20995, f3_072=25172)


def descale(x, n):
    return (x + (1 << (n - 1))) >> n


def fix(x):
    """jccolor / jdcolor: 16 fraction bits"""
    return int(x * 65536 + 0.5)


class Geometry:
    """Block geometry of a frame (the arithmetic csrc/jpeg_common.h: jpeg_grid repeats).  With ``restart_rows`` (the
    encoder, which writes ``WRITTEN_MODES`` only; 0: no markers) also its restart intervals and real luminance blocks
    (csrc/jpeg.hip: geometry)."""

    def __init__(self, H, W, mode, restart_rows=None):
        what, modes = ("mode", MODES) if restart_rows is None else ("subsampling", WRITTEN_MODES)
        if mode not in modes:
            raise ValueError(f"{what}: one of {modes}, got {mode!r}")
        H, W = int(H), int(W)
        if H < 1 or W < 1 or H > 65535 or W > 65535:
            raise ValueError(f"a JPEG frame is 1..65535 pixels a side, got {H}x{W}")
        self.H, self.W, self.mode = H, W, mode
        self.hs, self.vs = SAMPLING[mode]                              # luminance sampling: an MCU is 8 hs x 8 vs pixels
        self.ncomp = 1 if mode == "L" else 3
        self.blocks_per_mcu = 1 if mode == "L" else self.hs * self.vs + 2
        self.mcus_per_row, self.mcu_rows = -(-W // (8 * self.hs)), -(-H // (8 * self.vs))
        self.n_mcus = self.mcus_per_row * self.mcu_rows
        self.n_blocks = self.n_mcus * self.blocks_per_mcu
        self.comp_of = (0,) * (self.hs * self.vs) + ((1, 2) if self.ncomp == 3 else ())
        self.dw, self.dh = -(-W // self.hs), -(-H // self.vs)           # the chroma planes' real size
        if restart_rows is not None:
            self.restart_rows = int(restart_rows)
            if self.restart_rows < 0:
                raise ValueError("restart_rows >= 0")
            self.wib, self.hib = -(-W // 8), -(-H // 8)                 # real Y blocks
            self.rows_per_interval = self.restart_rows or self.mcu_rows
            self.n_intervals = -(-self.mcu_rows // self.rows_per_interval)
            self.restart_interval = self.restart_rows * self.mcus_per_row
            if self.restart_interval > 65535:
                raise ValueError("restart interval above 65535 MCUs")


def code_lengths(bits):
    """The canonical code assignment of Annex C, walked once: ``bits`` (number of codes of each length 1..16) -> for every
    length n (n, the first code of that length, the index in code order of its first symbol).  The bits[n-1] codes of a
    length are consecutive; the table assigns more codes than a length has when ``first + bits[n-1] > 1 << n``."""
    code = k = 0
    for n, b in enumerate(bits, 1):
        yield n, code, k
        code, k = (code + b) << 1, k + b


class InFlight:
    """Up to two submissions in flight on two alternating slots, oldest first: whose turn it is, the refusal of a third,
    the event behind a submission and the wait for the oldest.  What a slot holds is its owner's business."""

    def __init__(self, owner):
        self.owner, self.turn, self._queue = owner, 0, []

    def __len__(self):
        return len(self._queue)

    def slot(self):
        """The slot of the next submission."""
        if len(self._queue) == 2:
            raise RuntimeError(f"{self.owner}: two submissions are in flight; collect() one first")
        return self.turn

    def push(self, *what):
        """Behind what was queued for slot ``turn``: an event on the current stream; ``what`` comes back from ``pop``."""
        import torch
        event = torch.cuda.Event()
        event.record()
        self._queue.append((self.turn, event, what))
        self.turn ^= 1

    def pop(self):
        """Waits for the oldest submission -> (its slot, *what)."""
        if not self._queue:
            raise RuntimeError(f"{self.owner}: nothing was submitted")
        slot, event, what = self._queue.pop(0)
        event.synchronize()
        return (slot, *what)

    def require_idle(self, method):
        if self._queue:
            raise RuntimeError(f"{self.owner}.{method}: collect() what was submitted first")
