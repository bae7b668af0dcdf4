"""Baseline JPEG files as Pillow (libjpeg) writes them, restated in integers: the definition csrc/jpeg.hip is held to.

    jpeg_reference(frames_u8, quality=75, subsampling="4:2:0", restart_rows=1)      host only (numpy), byte-equal to
                                                                                     Image.save(..., "JPEG", quality=...,
                                                                                     subsampling=..., restart_marker_rows=...)
    JpegEncoder(device, height, width, ...)                                         the same files from the device

Baseline JPEG as libjpeg writes it is integer arithmetic end to end, so the contract is equality, as for the frame
scaler (ir2rgb_amd.transform.resize_reference / csrc/frame_scale.hip).  The rules, each in libjpeg's statement order:

tables    jpeg_set_quality(q, force_baseline): s = 5000 / q for q < 50 else 200 - 2 q; entry = clamp((base s + 50) / 100,
          1, 255) over the two Annex K base tables.  Huffman tables: Annex K.3 - K.6, never optimised.
colour    jccolor, 16 fraction bits, FIX(x) = int(x 65536 + 0.5):
          Y  = (FIX(.299) R + FIX(.587) G + FIX(.114) B + 32768) >> 16
          Cb = (-FIX(.16874) R - FIX(.33126) G + FIX(.5) B + (128 << 16) + 32767) >> 16
          Cr = (FIX(.5) R - FIX(.41869) G - FIX(.08131) B + (128 << 16) + 32767) >> 16          mode L: the byte itself
edges     every component is replicated to the right and downwards to its block grid.  For 4:2:0 the FULL-RESOLUTION chroma
          planes are extended first (one row when H is odd, columns up to twice the chroma block width), then
          downsampled h2v2: (a + b + c + d + bias) >> 2 with bias 1, 2, 1, 2 ... by output column, padded columns
          included; the downsampled rows are then replicated downwards.
DCT       jfdctint ("islow") in int32, CONST_BITS 13, PASS1_BITS 2, rows then columns, DESCALE(x, n) = (x + (1 << (n-1)))
          >> n, on sample - 128; the output is scaled by 8.
quantise  sign(c) ((|c| + (8 q >> 1)) / (8 q)), zigzag order.
dummies   4:2:0 with an odd number of Y block columns / rows: a block to the right of the last real block column has zero
          AC and the quantised DC of the block before it in the MCU; a block row below the last real one has zero AC and
          every DC equal to that of the last block of the preceding row of the MCU.
entropy   interleaved MCUs (Y x 4, Cb, Cr for 4:2:0; Y, Cb, Cr for 4:4:4; mode L non-interleaved); DC as the difference
          to the previous block of the component; AC (run, size) with ZRL 0xF0 and EOB 0x00; a negative value v is coded as
          v - 1 in ``size`` bits; 0x00 follows every 0xFF byte.
restart   every ``restart_rows`` MCU rows: pad with 1-bits to a byte, FF D0+(n mod 8), predictors reset.  The last
          interval is padded the same way and followed by FF D9.  The restart interval is the unit of parallelism of the
          device path, so ``restart_rows=0`` (no markers) exists in ``jpeg_reference`` only.
header    SOI, JFIF APP0 (1.01, units 0, density 1x1), one DQT per table, SOF0, one DHT per table, DRI, SOS.
shared    what the decoder (``jpeg_decode``) needs as well is stated once, in ``jpeg_common``.
"""
import numpy as np

from .jpeg_common import WRITTEN_MODES as MODES         # the index is the ``mode`` of include/ir2rgb_hip.h
from .jpeg_common import ZIGZAG, F, Geometry, InFlight, code_lengths, descale, fix

__all__ = ["jpeg_reference", "JpegEncoder", "quality_tables", "header", "MODES"]

BASE_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                      14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                      49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], dtype=np.int64)
BASE_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                        47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32, dtype=np.int64)

# Annex K.3 - K.6: (number of codes of each length 1..16, symbols in code order)
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d],
           [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32,
            0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16,
            0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45,
            0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
            0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94,
            0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
            0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8,
            0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
            0xf9, 0xfa])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77],
             [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81,
              0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34,
              0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44,
              0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
              0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92,
              0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
              0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
              0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
              0xf9, 0xfa])

# Faults a test plants to show that the equality check has teeth (tests/test_jpeg_cpu.py); empty in every other use.
#   quant_floor  chroma_bias_2  chroma_pad_output  dummy_real_dct  no_stuffing  no_predictor_reset
_FAULTS = frozenset()

COUNTERS = ("zrl", "stuffed", "max_dc_size", "max_ac_size", "eob_only_blocks", "dummy_right", "dummy_bottom", "odd_h_chroma_rows",
            "padded_chroma_cols_bias1", "padded_chroma_cols_bias2", "intervals", "rst_wrapped")


# ---------------------------------------------------------------------------------------------
# tables and header
# ---------------------------------------------------------------------------------------------
def quality_tables(quality):
    """jpeg_set_quality(quality, TRUE) -> (luminance, chrominance) int64 [64] in natural order."""
    q = min(max(int(quality), 1), 100)
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((base * s + 50) // 100, 1, 255) for base in (BASE_LUMA, BASE_CHROMA))


def huffman_codes(spec):
    """(bits, values) -> (code, length) int arrays indexed by symbol (length 0: no code), Annex C."""
    bits, vals = spec
    code, length = np.zeros(256, dtype=np.int64), np.zeros(256, dtype=np.int64)
    for n, first, k in code_lengths(bits):
        for j in range(bits[n - 1]):
            code[vals[k + j]], length[vals[k + j]] = first + j, n
    return code, length


def _segment(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def header(H, W, quality=75, subsampling="4:2:0", restart_rows=1):
    """Everything Pillow writes before the scan data, SOS included."""
    g = Geometry(H, W, subsampling, restart_rows)
    grey = subsampling == "L"
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for i, t in enumerate(quality_tables(quality)[:1 if grey else 2]):
        out += _segment(0xDB, bytes([i]) + bytes(int(v) for v in t[ZIGZAG]))
    comps = [(1, g.hs << 4 | g.vs, 0)] + ([] if grey else [(2, 0x11, 1), (3, 0x11, 1)])
    out += _segment(0xC0, bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([len(comps)])
                    + b"".join(bytes(c) for c in comps))
    for i, (dc, ac) in enumerate([(DC_LUMA, AC_LUMA), (DC_CHROMA, AC_CHROMA)][:1 if grey else 2]):
        out += _segment(0xC4, bytes([i]) + bytes(dc[0]) + bytes(dc[1]))
        out += _segment(0xC4, bytes([0x10 | i]) + bytes(ac[0]) + bytes(ac[1]))
    if g.restart_rows:
        out += _segment(0xDD, g.restart_interval.to_bytes(2, "big"))
    out += _segment(0xDA, bytes([len(comps)]) + b"".join(bytes([c[0], c[2] * 0x11]) for c in comps) + b"\x00\x3f\x00")
    return out


# ---------------------------------------------------------------------------------------------
# samples -> quantised blocks
# ---------------------------------------------------------------------------------------------
def _ycc(rgb):
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    y = (fix(.299) * r + fix(.587) * g + fix(.114) * b + 32768) >> 16
    cb = (-fix(.16874) * r - fix(.33126) * g + fix(.5) * b + (128 << 16) + 32767) >> 16
    cr = (fix(.5) * r - fix(.41869) * g - fix(.08131) * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def _extend(p, rows, cols):
    """Replicate the last row / column of a plane up to [rows, cols]."""
    return np.pad(p, ((0, rows - p.shape[0]), (0, cols - p.shape[1])), mode="edge")


def _h2v2(c, g, counters):
    """One full-resolution chroma plane [H, W] -> the downsampled plane on the chroma block grid."""
    out_cols, real_cols = 8 * g.mcus_per_row, -(-g.W // 2)
    rows = g.H + (g.H & 1)
    if "chroma_pad_output" in _FAULTS:
        c = _extend(c, rows, 2 * real_cols)
    else:
        c = _extend(c, rows, 2 * out_cols)
    bias = np.where(np.arange(c.shape[1] // 2) % 2 == 0, 1, 2)
    if "chroma_bias_2" in _FAULTS:
        bias = np.full_like(bias, 2)
    d = (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + bias[None, :]) >> 2
    counters["odd_h_chroma_rows"] += g.H & 1
    padded = np.arange(real_cols, out_cols)
    counters["padded_chroma_cols_bias1"] += int((padded % 2 == 0).sum())
    counters["padded_chroma_cols_bias2"] += int((padded % 2 == 1).sum())
    return _extend(d, 8 * g.mcu_rows, out_cols)


def _fdct_pass(d, first):
    """jfdctint's one-dimensional pass along the last axis of ``d`` int64 [..., 8]."""
    t0, t7, t1, t6 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7], d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5, t3, t4 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5], d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 13 - 2 if first else 13 + 2
    out = np.empty_like(d)
    if first:
        out[..., 0], out[..., 4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        out[..., 0], out[..., 4] = descale(t10 + t11, 2), descale(t10 - t11, 2)
    z1 = (t12 + t13) * F["f0_541"]
    out[..., 2] = descale(z1 + t13 * F["f0_765"], n)
    out[..., 6] = descale(z1 - t12 * F["f1_847"], n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * F["f1_175"]
    t4, t5, t6, t7 = t4 * F["f0_298"], t5 * F["f2_053"], t6 * F["f3_072"], t7 * F["f1_501"]
    z1, z2, z3, z4 = -z1 * F["f0_899"], -z2 * F["f2_562"], -z3 * F["f1_961"] + z5, -z4 * F["f0_390"] + z5
    out[..., 7] = descale(t4 + z1 + z3, n)
    out[..., 5] = descale(t5 + z2 + z4, n)
    out[..., 3] = descale(t6 + z2 + z3, n)
    out[..., 1] = descale(t7 + z1 + z4, n)
    return out


def _blocks(plane, qtab):
    """A plane on its block grid [8 hb, 8 wb] -> quantised coefficients int64 [hb, wb, 64] in zigzag order."""
    hb, wb = plane.shape[0] // 8, plane.shape[1] // 8
    d = plane.reshape(hb, 8, wb, 8).transpose(0, 2, 1, 3).astype(np.int64) - 128
    d = _fdct_pass(d, True)                                           # rows
    d = _fdct_pass(d.transpose(0, 1, 3, 2), False).transpose(0, 1, 3, 2)      # columns
    c = d.reshape(hb, wb, 64)
    div = (qtab.astype(np.int64) << 3)[None, None, :]
    half = 0 if "quant_floor" in _FAULTS else div >> 1
    q = np.sign(c) * ((np.abs(c) + half) // div)
    return q[:, :, ZIGZAG]


def scan_blocks(frame, g, quality, counters=None):
    """uint8 [H, W, C] -> the quantised blocks of the scan in coding order, int64 [n_blocks, 64] (zigzag)."""
    counters = counters if counters is not None else dict.fromkeys(COUNTERS, 0)
    ql, qc = quality_tables(quality)
    mr, mc = g.mcu_rows, g.mcus_per_row
    if g.mode == "L":
        return _blocks(_extend(frame[..., 0].astype(np.int64), 8 * mr, 8 * mc), ql).reshape(-1, 64)
    y, cb, cr = _ycc(frame)
    if g.mode == "4:4:4":
        comps = [_blocks(_extend(p, 8 * mr, 8 * mc), q) for p, q in ((y, ql), (cb, qc), (cr, qc))]
        return np.stack(comps, axis=2).reshape(-1, 64)
    if "dummy_real_dct" in _FAULTS:
        yb = _blocks(_extend(y, 16 * mr, 16 * mc), ql)
    else:
        yb = np.zeros((2 * mr, 2 * mc, 64), dtype=np.int64)
        yb[:g.hib, :g.wib] = _blocks(_extend(y, 8 * g.hib, 8 * g.wib), ql)
        if g.wib < 2 * mc:                                              # the block before it in the MCU
            yb[:g.hib, g.wib, 0] = yb[:g.hib, g.wib - 1, 0]
            counters["dummy_right"] += g.hib
        if g.hib < 2 * mr:                                              # the last block of the MCU's preceding row
            yb[g.hib, :, 0] = np.repeat(yb[g.hib - 1, 1::2, 0], 2)
            counters["dummy_bottom"] += 2 * mc
    cbb, crb = (_blocks(_h2v2(p, g, counters), qc) for p in (cb, cr))
    ym = yb.reshape(mr, 2, mc, 2, 64).transpose(0, 2, 1, 3, 4).reshape(mr, mc, 4, 64)
    return np.concatenate([ym, cbb[:, :, None], crb[:, :, None]], axis=2).reshape(-1, 64)


# ---------------------------------------------------------------------------------------------
# entropy coding
# ---------------------------------------------------------------------------------------------
class _Bits:
    def __init__(self, counters):
        self.out, self.acc, self.n, self.counters = bytearray(), 0, 0, counters

    def put(self, value, nbits):
        self.acc, self.n = (self.acc << nbits) | value, self.n + nbits
        while self.n >= 8:
            self.n -= 8
            byte = (self.acc >> self.n) & 0xFF
            self.out.append(byte)
            if byte == 0xFF:
                self.counters["stuffed"] += 1
                if "no_stuffing" not in _FAULTS:
                    self.out.append(0)
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _size(v):
    return int(abs(v)).bit_length()


def _encode_block(w, blk, pred, dc, ac, counters):
    diff = int(blk[0]) - pred
    s = _size(diff)
    counters["max_dc_size"] = max(counters["max_dc_size"], s)
    w.put(int(dc[0][s]), int(dc[1][s]))
    if s:
        w.put((diff if diff >= 0 else diff - 1) & ((1 << s) - 1), s)
    run = 0
    nz = np.flatnonzero(blk[1:]) + 1
    if nz.size == 0:
        counters["eob_only_blocks"] += 1
    last = 0
    for k in nz:
        run = int(k) - last - 1
        while run > 15:
            w.put(int(ac[0][0xF0]), int(ac[1][0xF0]))
            counters["zrl"] += 1
            run -= 16
        v = int(blk[k])
        s = _size(v)
        counters["max_ac_size"] = max(counters["max_ac_size"], s)
        w.put(int(ac[0][(run << 4) | s]), int(ac[1][(run << 4) | s]))
        w.put((v if v >= 0 else v - 1) & ((1 << s) - 1), s)
        last = int(k)
    if last < 63:
        w.put(int(ac[0][0]), int(ac[1][0]))


_CODES = None


def _codes():
    global _CODES
    if _CODES is None:
        _CODES = [(huffman_codes(DC_LUMA), huffman_codes(AC_LUMA)), (huffman_codes(DC_CHROMA), huffman_codes(AC_CHROMA))]
    return _CODES


def entropy_scan(blocks, g, counters):
    """The blocks of a scan in coding order -> the bytes after SOS, EOI included."""
    codes = _codes()
    per_interval = g.rows_per_interval * g.mcus_per_row * g.blocks_per_mcu
    w = _Bits(counters)
    pred = [0, 0, 0]
    for i in range(g.n_intervals):
        if "no_predictor_reset" not in _FAULTS:
            pred = [0, 0, 0]
        chunk = blocks[i * per_interval:(i + 1) * per_interval]
        for j, blk in enumerate(chunk):
            c = g.comp_of[j % g.blocks_per_mcu]
            dc, ac = codes[min(c, 1)]
            _encode_block(w, blk, pred[c], dc, ac, counters)
            pred[c] = int(blk[0])
        w.flush()
        last = i == g.n_intervals - 1
        w.out += bytes([0xFF, 0xD9 if last else 0xD0 + (i & 7)])
    counters["intervals"] += g.n_intervals
    counters["rst_wrapped"] += int(g.n_intervals > 9)                  # marker n = 8 is FF D0 again
    return bytes(w.out)


def _as_frames(frames_u8):
    a = frames_u8.detach().cpu().numpy() if hasattr(frames_u8, "detach") else np.asarray(frames_u8)
    if a.dtype != np.uint8:
        raise TypeError(f"uint8 frames expected, got {a.dtype}")
    if a.ndim == 3:
        a = a[None]
    if a.ndim != 4 or a.shape[3] not in (1, 3):
        raise ValueError(f"frames [N,H,W,C] with C in (1, 3) expected, got {a.shape}")
    return a


def jpeg_reference(frames_u8, quality=75, subsampling="4:2:0", restart_rows=1, counters=False):
    """uint8 [N,H,W,C] (C in {1, 3}; or one [H,W,C] frame) -> the JPEG file of every frame as Pillow writes it
    (``Image.save(f, "JPEG", quality=quality, subsampling=subsampling, restart_marker_rows=restart_rows)``; mode L for
    ``subsampling="L"``, which encodes channel 0).  ``counters=True`` -> (files, dict of the paths the streams took: the
    names of ``COUNTERS``)."""
    a = _as_frames(frames_u8)
    if subsampling != "L" and a.shape[3] != 3:
        raise ValueError(f"subsampling {subsampling!r} needs three channels")
    g = Geometry(a.shape[1], a.shape[2], subsampling, restart_rows)
    cnt = dict.fromkeys(COUNTERS, 0)
    head = header(g.H, g.W, quality, subsampling, restart_rows)
    files = [head + entropy_scan(scan_blocks(f, g, quality, cnt), g, cnt) for f in a]
    return (files, cnt) if counters else files


# ---------------------------------------------------------------------------------------------
# the device path
# ---------------------------------------------------------------------------------------------
TABLE_WORDS = 128 + 32 + 512


def device_tables(quality):
    """The words csrc/jpeg.hip reads, from the objects ``header`` writes: quantisation [2][64] (natural order), DC codes
    [2][16] and AC codes [2][256] as ``length << 16 | code`` -> (uint32 [672], longest DC code, longest AC code)."""
    t = np.zeros(TABLE_WORDS, dtype=np.uint32)
    for i, q in enumerate(quality_tables(quality)):
        t[64 * i:64 * i + 64] = q
    for i, ((dcode, dlen), (acode, alen)) in enumerate(_codes()):
        t[128 + 16 * i:128 + 16 * i + 16] = (dlen[:16] << 16) | dcode[:16]
        t[160 + 256 * i:160 + 256 * i + 256] = (alen << 16) | acode
    return t, int(max(c[0][1].max() for c in _codes())), int(max(c[1][1].max() for c in _codes()))


_COPY_STREAMS = {}


def fetch(src, pinned):
    """The bytes of a finished device tensor through a pinned staging buffer, on a copy stream of its own: the caller has
    waited for the event behind ``src``, and the copy must not queue behind whatever the current stream was given since."""
    import torch
    stream = _COPY_STREAMS.get(src.device)
    if stream is None:
        stream = _COPY_STREAMS[src.device] = torch.cuda.Stream(src.device)
    m = src.numel()
    with torch.cuda.stream(stream):
        pinned[:m].copy_(src, non_blocking=True)
    stream.synchronize()
    return pinned[:m].numpy().tobytes()


def fetch_file(row, length, pinned, who, floor=0, note=""):
    """The file in the device row ``row`` whose size the device reported as ``length`` (read from pinned memory, after the
    event behind both): the size is held to ``floor < length <= len(row)`` before ``fetch`` copies that many bytes."""
    m = int(length)
    if not floor < m <= row.shape[0]:
        raise RuntimeError(f"{who} reports {m} bytes{note}")
    return fetch(row[:m], pinned)


class JpegEncoder:
    """JPEG files of uint8 device frames, encoded on the device (csrc/jpeg.hip), equal to ``jpeg_reference`` byte for byte.

        enc = JpegEncoder(device, height, width)                 # Pillow's defaults: quality 75, 4:2:0
        files = enc.encode(frames_u8)                            # [N,H,W,C] or [H,W,C] -> list of bytes (synchronises)
        enc.submit(frames_k); ...; files = enc.collect()         # pipelined: collect() hands back the submission before

    ``submit`` queues three launches, the copy of the N lengths into pinned memory and an event on the current stream and
    returns; it never waits.  ``collect`` waits for that event and copies exactly ``length`` bytes per file.  Two
    submissions may be in flight (two device outputs, two pinned staging buffers, as ``Snapshots``): a third ``submit``
    without a ``collect`` raises.  ``channels=3`` with ``subsampling="L"`` encodes channel 0 of three-channel frames (a
    one-channel snapshot panel inside the [P,H,W,3] stack).  The header is built once here; quantisation and Huffman tables
    go to the device from the same objects."""

    def __init__(self, device, height, width, channels=3, quality=75, subsampling="4:2:0", restart_rows=1):
        import torch
        from . import _lib
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("JpegEncoder runs on an AMD GPU only (jpeg_reference is the host definition)")
        if int(restart_rows) < 1:
            raise ValueError("JpegEncoder: restart_rows >= 1 (the restart interval is the unit of parallelism; "
                             "jpeg_reference writes files without markers)")
        if channels not in (1, 3) or (subsampling != "L" and channels != 3):
            raise ValueError(f"JpegEncoder: channels {channels} does not fit subsampling {subsampling!r}")
        self.geometry = Geometry(height, width, subsampling, restart_rows)
        self.H, self.W, self.C = int(height), int(width), int(channels)
        self.quality, self.subsampling, self.restart_rows = int(quality), subsampling, int(restart_rows)
        self.mode = MODES.index(subsampling)
        self.header = header(self.H, self.W, self.quality, subsampling, self.restart_rows)
        words, self.max_dc, self.max_ac = device_tables(self.quality)
        self._tables = torch.from_numpy(words.view(np.int32)).to(self.device)
        self._header = torch.frombuffer(bytearray(self.header), dtype=torch.uint8).to(self.device)
        self.capacity = _lib.query("ir2rgb_jpeg_capacity_bytes", self.H, self.W, self.mode, self.restart_rows, len(self.header),
                                   self.max_dc, self.max_ac)
        self._n = 0
        self._slots = [None, None]       # per slot: (out [n, capacity], lengths [n], pinned lengths, pinned bytes)
        self._ws = None
        self._pending = InFlight("JpegEncoder")         # remembers n
        self.in_flight = self._pending                  # public: len() is the submissions collect() has not handed back
        # (nothing but header and tables is allocated before the first submit())

    def workspace_bytes(self, n):
        from . import _lib
        return _lib.query("ir2rgb_jpeg_workspace_bytes", n, self.H, self.W, self.mode, self.restart_rows, self.max_dc, self.max_ac)

    def _reserve(self, n, slot=None):
        """Room for ``n`` frames: the workspace (shared by all launches of the one stream this encoder is used on; a larger
        one replaces it, and the allocator keeps the old block from work queued later only) and, with ``slot``, that
        slot's output and staging.  The slot about to be used is never in flight."""
        import torch
        dev = self.device
        if n > self._n:
            self._ws = torch.empty(self.workspace_bytes(n), dtype=torch.uint8, device=dev)
            self._n = n
        if slot is not None and (self._slots[slot] is None or self._slots[slot][0].shape[0] < n):
            self._slots[slot] = (torch.empty((n, self.capacity), dtype=torch.uint8, device=dev),
                                 torch.empty(n, dtype=torch.int32, device=dev),
                                 torch.empty(n, dtype=torch.int32, pin_memory=True),
                                 torch.empty(self.capacity, dtype=torch.uint8, pin_memory=True))

    def _frames(self, frames_u8):
        import torch
        from . import _lib
        f = frames_u8.unsqueeze(0) if frames_u8.dim() == 3 else frames_u8
        _lib.require_device(f, dtype=torch.uint8)
        if f.dim() != 4 or tuple(f.shape[1:]) != (self.H, self.W, self.C) or f.shape[0] < 1:
            raise ValueError(f"JpegEncoder: frames [N,{self.H},{self.W},{self.C}] expected, got {tuple(frames_u8.shape)}")
        if f.device != self.device:
            raise ValueError(f"JpegEncoder: frames on {f.device}, the encoder is on {self.device}")
        return f

    def encode_into(self, frames, out, lengths, workspace=None):
        """The launches alone, on the current stream: ``frames`` [N,H,W,C] -> files in ``out`` uint8 [N, >= capacity] and
        their sizes in ``lengths`` int32 [N] (device tensors)."""
        from . import _lib
        if workspace is None:
            self._reserve(frames.shape[0])
        ws = self._ws if workspace is None else workspace
        _lib.launch("ir2rgb_jpeg_encode_u8", frames, frames, out, lengths, ws, ws.numel(), self._header, len(self.header),
                    self._tables, frames.shape[0], self.C, self.H, self.W, self.mode, self.restart_rows, self.max_dc, self.max_ac,
                    out.shape[1])

    def submit(self, frames_u8):
        import torch
        f = self._frames(frames_u8)
        slot = self._pending.slot()
        self._reserve(f.shape[0], slot)
        out, lengths, host_len, _ = self._slots[slot]
        n = f.shape[0]
        with torch.cuda.device(self.device):
            # the workspace is shared: launches of one stream run in order, and submit() is a one-stream interface
            self.encode_into(f, out[:n], lengths[:n])
            host_len[:n].copy_(lengths[:n], non_blocking=True)
            self._pending.push(n)

    def collect(self):
        """The files of the oldest submission in flight."""
        slot, n = self._pending.pop()
        out, _, host_len, host = self._slots[slot]
        return [fetch_file(out[i], host_len[i], host, f"JpegEncoder: frame {i}", len(self.header), f" (capacity {self.capacity})")
                for i in range(n)]

    def encode(self, frames_u8):
        self._pending.require_idle("encode")
        self.submit(frames_u8)
        return self.collect()
