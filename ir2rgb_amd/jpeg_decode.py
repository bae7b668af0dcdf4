"""Baseline JPEG files decoded as Pillow (libjpeg-turbo) decodes them, restated in integers: the definition
csrc/jpeg_decode.hip is held to.

    parse(data)                      header -> Info: geometry, tables, the scan cut into segments (restart intervals)
    decode_reference(data)           host only (numpy), equal to np.asarray(Image.open(...)) pixel for pixel
    entropy_model(info, sub_bytes)   the parallel entropy decode of the kernel's first phase, in plain Python
    JpegDecoder(device, H, W, mode)  the same pixels from the device

Baseline decoding is integer arithmetic end to end, so the contract is equality, as for ``jpeg.jpeg_reference``.  The rules:

entropy   canonical Huffman codes (Annex C); a value v of s bits is v - 2^s + 1 when v < 2^(s-1); DC is a running sum per
          component, reset at every restart marker; AC (run, size) with ZRL 0xF0 and EOB 0x00; the 00 after an FF byte is
          stuffing.  A byte is stuffing exactly when it is 00 and the raw byte before it (inside the segment) is FF.
dequant   coefficient * q, natural order.
IDCT      jpeg_idct_islow: CONST_BITS 13, PASS1_BITS 2, columns first with DESCALE(x, 11), then rows with DESCALE(x, 18),
          + 128, clamp to 0..255.
upsample  on the component's real downsampled size dw = ceil(W/2), dh = ceil(H/2).  dw <= 2: plain replication.  Otherwise
          h2v2 "fancy": colsum = 3 near_row + far_row (far: the row above for even output rows, below for odd ones; row -1
          is row 0, row dh is row dh-1); out[2i] = (3 this + last + 8) >> 4, out[2i+1] = (3 this + next + 7) >> 4 with
          last = this in the first column and next = this in the last.  h2v1 fancy (4:2:2): out[2i] = (3 this + last + 1)
          >> 2, out[2i+1] = (3 this + next + 2) >> 2, out[0] = in[0], out[2dw-1] = in[dw-1].
colour    jdcolor, FIX(x) = int(x 65536 + 0.5) on cb - 128, cr - 128: R = y + ((FIX(1.402) cr + 32768) >> 16),
          B = y + ((FIX(1.772) cb + 32768) >> 16), G = y + ((-FIX(.34414) cb + 32768 - FIX(.71414) cr) >> 16), clamped.

The parallel entropy decode (``entropy_model``, csrc/jpeg_decode.hip).  A segment's raw, still-stuffed bytes are cut into
subsequences of ``sub_bytes``.  A decoder state between two symbols is (bit position, block within the MCU, zigzag
position k); positions count raw bits from the segment's start and never point into a stuffing byte.  Subsequence 0
enters at the true state (0, 0, 0), every other one at a guess: its first byte, block 0, k = 0.  In a round every
subsequence decodes the symbols that START inside it and hands its exit state to its right neighbour (a subsequence whose
entry lies at or past its own end decodes nothing and hands the entry on).  After round r the entries of subsequences 0..r
are the true ones, so at most n_sub rounds are needed; a round that changes no entry ends the loop earlier -- Huffman
streams resynchronise, so that is the usual end.  Wrong-sync decodes read garbage by design: reads past the segment's end
give 1-bits, 16 bits that are no code are consumed as symbol 0, k never passes 64.
What the encoder (``jpeg``) needs as well is stated once, in ``jpeg_common``.
"""
import os

import numpy as np

from .jpeg_common import MODES, SAMPLING, ZIGZAG, F, Geometry, InFlight, code_lengths, descale, fix

__all__ = ["parse", "decode_reference", "entropy_model", "JpegDecoder", "MODES", "Info", "Segment"]

_LUMA_SAMPLING = {hv: mode for mode, hv in SAMPLING.items() if mode != "L"}       # of a three-component frame

# status bits of the write pass (include/ir2rgb_hip.h: IR2RGB_JPEGD_*)
ERR_CODE, ERR_INDEX, ERR_BLOCKS, ERR_LEFTOVER, ERR_SEGMENT = 1, 2, 4, 8, 16
ERR_NAMES = {ERR_CODE: "invalid Huffman code", ERR_INDEX: "coefficient index past 63", ERR_BLOCKS: "block count differs from the segment's",
             ERR_LEFTOVER: "bits left over beyond the padding", ERR_SEGMENT: "segment record outside the frame"}

ENT_THREADS = 512               # subsequences one workgroup of jpegd_entropy_kernel takes (one thread each)
DEFAULT_SUB_BYTES = 128         # DESIGN.md "JPEG input": the choice and what it rests on
TABLE_WORDS = 192 + 8 + 4 * 288

# Faults a test plants to show that the equality check has teeth (tests/test_jpeg_decode_cpu.py); empty in every other use.
#   fancy_narrow  bias_swapped  far_row_top  no_predictor_reset  dc_across_components  fix_floor  no_unstuffing
_FAULTS = frozenset()

COUNTERS = ("zrl", "stuffed", "code16", "eob_only_blocks", "segments", "rst_wrapped", "narrow_chroma", "odd_h", "odd_w",
            "top_context", "bottom_context", "boundary_on_stuffing", "short_segment", "enlarged")


def _counters():
    return dict.fromkeys(COUNTERS, 0)


# ---------------------------------------------------------------------------------------------
# header
# ---------------------------------------------------------------------------------------------
class Segment:
    """One restart interval of the scan: MCUs [first_mcu, first_mcu + n_mcus), bytes [begin, end) of the file, the marker
    excluded."""
    __slots__ = ("first_mcu", "n_mcus", "begin", "end")

    def __init__(self, first_mcu, n_mcus, begin, end):
        self.first_mcu, self.n_mcus, self.begin, self.end = first_mcu, n_mcus, begin, end

    def __repr__(self):
        return f"Segment(mcu {self.first_mcu}+{self.n_mcus}, bytes {self.begin}:{self.end})"


class Info:
    """What ``parse`` reads of a file.  ``components``: [(id, h, v, quantisation table id, dc table id, ac table id)];
    ``qtables``: {id: int64 [64] natural order}; ``huffman``: {(class, id): (bits [16], values)}, class 0 = DC."""

    def __init__(self):
        self.H = self.W = 0
        self.components, self.qtables, self.huffman = [], {}, {}
        self.restart_interval = 0
        self.scan = (0, 0)
        self.segments = []
        self.data = b""

    @property
    def mode(self):
        return "L" if len(self.components) == 1 else _LUMA_SAMPLING[self.components[0][1:3]]

    @property
    def geometry(self):
        return Geometry(self.H, self.W, self.mode)


def _be16(d, i):
    if i + 2 > len(d):
        raise ValueError("JPEG: the header ends inside a segment")
    return (d[i] << 8) | d[i + 1]


_SOF_NAMES = {0xC1: "extended sequential (SOF1)", 0xC2: "progressive (SOF2)", 0xC3: "lossless (SOF3)", 0xC5: "differential (SOF5)",
              0xC6: "differential progressive (SOF6)", 0xC7: "differential lossless (SOF7)", 0xC9: "arithmetic coding (SOF9)",
              0xCA: "arithmetic progressive (SOF10)", 0xCB: "arithmetic lossless (SOF11)", 0xCD: "arithmetic (SOF13)",
              0xCE: "arithmetic (SOF14)", 0xCF: "arithmetic (SOF15)"}


def parse(data, strict=True):
    """The header of a baseline JPEG file and its scan cut into segments.  ``strict=False`` accepts a scan whose number of
    restart intervals is not the frame's (a damaged file: the device reports it in ``status``)."""
    d = bytes(data)
    if len(d) < 4 or d[0] != 0xFF or d[1] != 0xD8:
        raise ValueError("JPEG: no SOI marker (not a JPEG file)")
    info = Info()
    info.data = d
    i, sof, jfif, adobe = 2, False, False, None
    while True:
        if i + 2 > len(d):
            raise ValueError("JPEG: the file ends before the scan (truncated header)")
        if d[i] != 0xFF:
            raise ValueError(f"JPEG: marker expected at byte {i}, found {d[i]:#04x}")
        m = d[i + 1]
        if m == 0xFF:                                   # fill byte
            i += 1
            continue
        if m == 0xD9:
            raise ValueError("JPEG: EOI before any scan")
        n = _be16(d, i + 2)
        if n < 2 or i + 2 + n > len(d):
            raise ValueError(f"JPEG: segment {m:#04x} at byte {i} runs past the end of the file (truncated header)")
        p = d[i + 4:i + 2 + n]
        if m == 0xC0:
            if sof:
                raise ValueError("JPEG: two frame headers")
            if len(p) < 6:
                raise ValueError("JPEG: malformed SOF0")
            if p[0] != 8:
                raise NotImplementedError(f"JPEG: {p[0]}-bit samples (8-bit only)")
            info.H, info.W, nc = (p[1] << 8) | p[2], (p[3] << 8) | p[4], p[5]
            if nc not in (1, 3):
                raise NotImplementedError(f"JPEG: {nc} components (1 or 3 only)")
            if len(p) != 6 + 3 * nc:
                raise ValueError("JPEG: malformed SOF0")
            if info.H == 0 or info.W == 0:
                raise ValueError("JPEG: empty frame")
            comps = [(p[6 + 3 * c], p[7 + 3 * c] >> 4, p[7 + 3 * c] & 15, p[8 + 3 * c]) for c in range(nc)]
            if nc == 1:
                comps = [(comps[0][0], 1, 1, comps[0][3])]              # a single component is never interleaved
            elif (comps[0][1], comps[0][2]) not in _LUMA_SAMPLING or any(c[1:3] != (1, 1) for c in comps[1:]):
                raise NotImplementedError("JPEG: sampling factors " + ", ".join(f"{c[1]}x{c[2]}" for c in comps)
                                          + " (luminance 1x1, 2x1 or 2x2 with 1x1 chroma only)")
            info.components = comps
            sof = True
        elif m in _SOF_NAMES:
            raise NotImplementedError(f"JPEG: {_SOF_NAMES[m]} (baseline SOF0 only)")
        elif m == 0xCC:
            raise NotImplementedError("JPEG: arithmetic coding (DAC)")
        elif m == 0xDB:
            j = 0
            while j < len(p):
                if p[j] >> 4:
                    raise NotImplementedError("JPEG: 16-bit quantisation table")
                if j + 65 > len(p):
                    raise ValueError("JPEG: malformed DQT")
                t = np.zeros(64, dtype=np.int64)
                t[ZIGZAG] = np.frombuffer(p[j + 1:j + 65], dtype=np.uint8)
                info.qtables[p[j] & 15] = t
                j += 65
        elif m == 0xC4:
            j = 0
            while j < len(p):
                if j + 17 > len(p):
                    raise ValueError("JPEG: malformed DHT")
                cls, tid = p[j] >> 4, p[j] & 15
                bits = list(p[j + 1:j + 17])
                nv = sum(bits)
                if cls > 1 or nv > 256 or j + 17 + nv > len(p):
                    raise ValueError("JPEG: malformed DHT")
                if tid > 1:
                    raise NotImplementedError(f"JPEG: Huffman table id {tid} (0..1 only)")
                if any(first + bits[n_l - 1] > 1 << n_l for n_l, first, _ in code_lengths(bits)):
                    raise ValueError("JPEG: DHT assigns more codes than a length has")
                info.huffman[(cls, tid)] = (bits, list(p[j + 17:j + 17 + nv]))
                j += 17 + nv
        elif m == 0xDD:
            if len(p) != 2:
                raise ValueError("JPEG: malformed DRI")
            info.restart_interval = (p[0] << 8) | p[1]
        elif m == 0xE0 and p[:5] == b"JFIF\x00":
            jfif = True
        elif m == 0xEE and p[:5] == b"Adobe" and len(p) >= 12:
            adobe = p[11]
        elif m == 0xDA:
            if not sof:
                raise ValueError("JPEG: scan before the frame header")
            if len(p) < 1:
                raise ValueError("JPEG: malformed SOS")
            if p[0] != len(info.components):
                raise NotImplementedError(f"JPEG: a scan of {p[0]} of {len(info.components)} components (one interleaved scan only)")
            if len(p) != 4 + 2 * p[0]:
                raise ValueError("JPEG: malformed SOS")
            comps = []
            for c, comp in enumerate(info.components):
                if p[1 + 2 * c] != comp[0]:
                    raise NotImplementedError("JPEG: scan components in another order than the frame's")
                td, ta = p[2 + 2 * c] >> 4, p[2 + 2 * c] & 15
                if td > 1 or ta > 1:
                    raise NotImplementedError(f"JPEG: Huffman table id {max(td, ta)} (0..1 only)")
                if (0, td) not in info.huffman or (1, ta) not in info.huffman or comp[3] not in info.qtables:
                    raise ValueError("JPEG: the scan names a table the file does not define")
                comps.append(comp + (td, ta))
            if tuple(p[-3:]) != (0, 63, 0):
                raise NotImplementedError("JPEG: spectral selection / successive approximation (progressive)")
            info.components = comps
            i += 2 + n
            break
        # every other segment (APPn with EXIF, COM ...) is skipped
        i += 2 + n
    if len(info.components) == 3:
        # default_decompress_parms: JFIF says YCbCr; else Adobe's transform flag; else the component ids
        ids = tuple(c[0] for c in info.components)
        rgb = (not jfif) and ((adobe == 0) if adobe is not None else ids == (0x52, 0x47, 0x42))
        if rgb:
            raise NotImplementedError("JPEG: RGB-coded file (YCbCr and grayscale only)")
    # the scan: up to the first marker that is neither stuffing nor RSTn
    a = np.frombuffer(d, dtype=np.uint8)
    ff = np.flatnonzero(a[i:len(d) - 1] == 0xFF) + i
    nxt = a[ff + 1]
    marks = ff[nxt != 0]
    g = info.geometry
    ri = info.restart_interval or g.n_mcus
    begin, end, k = i, len(d), 0
    for mpos in marks:
        mk = int(a[mpos + 1])
        if mk == 0xFF:
            continue
        if 0xD0 <= mk <= 0xD7:
            first = min(k * ri, g.n_mcus)
            info.segments.append(Segment(first, min(ri, g.n_mcus - first), begin, int(mpos)))
            begin, k = int(mpos) + 2, k + 1
            continue
        end = int(mpos)
        break
    first = min(k * ri, g.n_mcus)
    info.segments.append(Segment(first, min(ri, g.n_mcus - first), begin, end))
    info.scan = (i, end)
    if strict:
        if d[end:end + 2] == b"\xff\xda" or d[end:end + 2] == b"\xff\xc4" or d[end:end + 2] == b"\xff\xdb":
            raise NotImplementedError("JPEG: several scans")
        if sum(s.n_mcus for s in info.segments) != g.n_mcus or len(info.segments) != -(-g.n_mcus // ri):
            raise ValueError(f"JPEG: {len(info.segments)} restart intervals in the scan, the frame has {-(-g.n_mcus // ri)}")
    return info


# ---------------------------------------------------------------------------------------------
# entropy decoding
# ---------------------------------------------------------------------------------------------
def huffman_decode_table(spec):
    """(bits, values) -> (limit uint32 [16], offset int32 [16], values int32 [256]): the code of a 16-bit window ``w`` has
    the smallest length l with w < limit[l-1], and its symbol is values[offset[l-1] + (w >> (16 - l))].  What the device
    reads (the per-file table block) and what ``_lut`` expands."""
    bits, vals = spec
    limit, offset = np.zeros(16, dtype=np.int64), np.zeros(16, dtype=np.int64)
    last = 0
    for n, first, k in code_lengths(bits):
        offset[n - 1] = k - first
        if bits[n - 1]:
            last = (first + bits[n - 1]) << (16 - n)
        limit[n - 1] = last
    values = np.zeros(256, dtype=np.int64)
    values[:len(vals)] = vals
    return limit, offset, values


def _lut(spec):
    """-> (length uint8 [65536], symbol uint8 [65536]) by 16-bit window; length 0: no code."""
    limit, offset, values = huffman_decode_table(spec)
    length, sym = np.zeros(65536, dtype=np.uint8), np.zeros(65536, dtype=np.uint8)
    lo = 0
    for n in range(1, 17):
        hi = int(limit[n - 1])
        if hi > lo:
            w = np.arange(lo, hi)
            length[lo:hi] = n
            sym[lo:hi] = values[np.clip(offset[n - 1] + (w >> (16 - n)), 0, 255)]
            lo = hi
    return length.tolist(), sym.tolist()


class _SegmentBits:
    """The data bytes of a segment (stuffing taken out), followed by FF bytes, and the raw position of every one."""

    def __init__(self, info, seg, counters=None):
        raw = np.frombuffer(info.data, dtype=np.uint8)[seg.begin:seg.end]
        self.n_raw = len(raw)
        keep = np.ones(len(raw), dtype=bool)
        if "no_unstuffing" not in _FAULTS:
            keep[1:] = ~((raw[1:] == 0) & (raw[:-1] == 0xFF))
        if counters is not None:
            counters["stuffed"] += int((~keep).sum())
        self.stuffing = ~keep
        self.raw_of = np.concatenate([np.flatnonzero(keep), self.n_raw + np.arange(8)])
        self.n_data = int(keep.sum())
        self.bytes = raw[keep].tobytes() + b"\xff" * 8
        self.end_bit = 8 * self.n_data

    def raw_bit(self, p):
        """data bit position -> raw bit position"""
        u = p >> 3
        r = int(self.raw_of[u]) if u < len(self.raw_of) else self.n_raw + (u - self.n_data)
        return 8 * r + (p & 7)

    def first_data_byte(self, raw_index):
        """the data byte index of the first data byte at or after a raw byte index"""
        return int(np.searchsorted(self.raw_of[:self.n_data], raw_index))


def _decode_symbols(sb, luts, g, comps, p, blk, k, end_bit, on_coef=None, stop_blocks=None, first_block=0, counters=None):
    """Decode the symbols that start in [p, end_bit) of a segment from the state (p, blk, k) (data bit coordinates).
    ``on_coef(block, k, value)`` for the write pass; ``stop_blocks``: stop (and look at what is left) once that many blocks
    are complete.  -> (p, blk, k, blocks completed, status)."""
    d = sb.bytes
    done, status = 0, 0
    bpm = g.blocks_per_mcu
    while p < end_bit:
        if stop_blocks is not None and first_block + done >= stop_blocks:
            if sb.end_bit - p > 7:
                status |= ERR_LEFTOVER
            break
        comp = comps[g.comp_of[blk]]
        length, sym = luts[(0 if k == 0 else 1, comp[4] if k == 0 else comp[5])]
        j, b = p >> 3, p & 7
        w = (int.from_bytes(d[j:j + 6], "big") << b) & 0xFFFFFFFFFFFF       # p < end_bit: the 8 FF bytes behind cover it
        peek = w >> 32
        n = length[peek]
        if n == 0:
            n, s_ = 16, 0
            if on_coef is not None:
                status |= ERR_CODE
        else:
            s_ = sym[peek]
            if counters is not None and n == 16:
                counters["code16"] += 1
        if k == 0:
            s = min(s_, 16)
            run = 0
        else:
            s, run = s_ & 15, s_ >> 4
        v = ((w << n) & 0xFFFFFFFFFFFF) >> (48 - s) if s else 0            # the s bits after the code
        p += n + s
        if s and v < (1 << (s - 1)):
            v = v - (1 << s) + 1
        if k == 0:
            if on_coef is not None:
                on_coef(first_block + done, 0, v)
            k = 1
        elif s:
            k += run
            if k > 63:
                if on_coef is not None:
                    status |= ERR_INDEX
                k = 64
            else:
                if on_coef is not None:
                    on_coef(first_block + done, k, v)
                k += 1
        elif run == 15:
            if counters is not None:
                counters["zrl"] += 1
            k += 16
            if k > 64:
                if on_coef is not None:
                    status |= ERR_INDEX
                k = 64
        else:
            if counters is not None and k == 1:
                counters["eob_only_blocks"] += 1
            k = 64
        if k >= 64:
            k, blk, done = 0, (blk + 1) % bpm, done + 1
    return p, blk, k, done, status


def effective_sub_bytes(seg_bytes, sub_bytes):
    """The subsequence size the kernel uses for a segment: ``sub_bytes``, enlarged until ENT_THREADS subsequences cover it."""
    return max(int(sub_bytes), -(-int(seg_bytes) // ENT_THREADS), 1)


def _luts(info):
    return {key: _lut(spec) for key, spec in info.huffman.items()}


def sequential_states(info, seg, sub_bytes, luts=None):
    """The true entry state of every subsequence of a segment, from one sequential decode: [(raw bit, blk, k)]."""
    g, luts = info.geometry, luts or _luts(info)
    sb = _SegmentBits(info, seg)
    sub = effective_sub_bytes(sb.n_raw, sub_bytes)
    n_sub = max(-(-sb.n_raw // sub), 1)
    states, p, blk, k = [], 0, 0, 0
    for j in range(n_sub):
        states.append((sb.raw_bit(p), blk, k))
        end = 8 * sb.first_data_byte(min((j + 1) * sub, sb.n_raw)) if j + 1 < n_sub else sb.end_bit
        p, blk, k, _, _ = _decode_symbols(sb, luts, g, info.components, p, blk, k, end)
    return states


def entropy_model(info, sub_bytes=DEFAULT_SUB_BYTES, counters=None, coefficients=False):
    """The kernel's parallel entropy decode of every segment, in plain Python.

    -> list over segments of dict(entries=[(raw bit, blk, k)], rounds=int, n_sub=int, sub_bytes=int, status=int
    [, blocks=int16 [n_blocks_of_segment, 64] natural order, DC still a difference])."""
    g, luts = info.geometry, _luts(info)
    out = []
    total = g.n_mcus
    for seg in info.segments:
        status = 0
        first, n_mcus = seg.first_mcu, seg.n_mcus
        if first < 0 or n_mcus < 0 or first + n_mcus > total:
            status |= ERR_SEGMENT
            first = min(max(first, 0), total)
            n_mcus = min(max(n_mcus, 0), total - first)
        if n_mcus == 0:                                     # an unused record
            out.append(dict(entries=[], rounds=0, n_sub=0, sub_bytes=0, status=status))
            continue
        seg_blocks = n_mcus * g.blocks_per_mcu
        sb = _SegmentBits(info, seg, counters)
        sub = effective_sub_bytes(sb.n_raw, sub_bytes)
        n_sub = max(-(-sb.n_raw // sub), 1)
        if counters is not None:
            counters["enlarged"] += int(sub > sub_bytes)
            counters["short_segment"] += int(sb.n_raw < sub)
            counters["boundary_on_stuffing"] += int(sum(bool(sb.stuffing[j * sub]) for j in range(1, n_sub)))
        starts = [8 * sb.first_data_byte(j * sub) for j in range(n_sub)]
        ends = starts[1:] + [sb.end_bit]
        entry = [(starts[j], 0, 0) for j in range(n_sub)]
        exits, counts = [None] * n_sub, [0] * n_sub
        dirty = [True] * n_sub
        rounds = 0
        for _ in range(n_sub):
            rounds += 1
            for j in range(n_sub):
                if dirty[j]:
                    p, blk, k, done, _ = _decode_symbols(sb, luts, g, info.components, *entry[j], ends[j])
                    exits[j], counts[j] = (p, blk, k), done
            changed = False
            dirty = [False] * n_sub
            for j in range(n_sub - 1):
                if exits[j] != entry[j + 1]:
                    entry[j + 1], dirty[j + 1], changed = exits[j], True, True
            if not changed:
                break
        if sum(counts) != seg_blocks:
            status |= ERR_BLOCKS
        rec = dict(entries=[(sb.raw_bit(p), blk, k) for p, blk, k in entry], rounds=rounds, n_sub=n_sub, sub_bytes=sub)
        # the write pass: from the true states, every subsequence stores what it decodes
        blocks = np.zeros((seg_blocks, 64), dtype=np.int64)

        def store(b, k, v):
            if b < seg_blocks:
                blocks[b, ZIGZAG[k]] = v
        before = 0
        for j in range(n_sub):
            status |= _decode_symbols(sb, luts, g, info.components, *entry[j], ends[j], on_coef=store, stop_blocks=seg_blocks,
                                      first_block=before, counters=counters)[4]
            before += counts[j]
        rec["status"] = status
        if coefficients:
            rec["blocks"] = blocks.astype(np.int16)
        out.append(rec)
    return out


def scan_coefficients(info, counters=None):
    """Sequential entropy decode -> int64 [n_blocks, 64], natural order, DC predicted (the definition)."""
    g, luts = info.geometry, _luts(info)
    blocks = np.zeros((g.n_blocks, 64), dtype=np.int64)
    across = "dc_across_components" in _FAULTS
    pred = [0, 0, 0]
    for seg in info.segments:
        sb = _SegmentBits(info, seg, counters)
        n = seg.n_mcus * g.blocks_per_mcu
        base = seg.first_mcu * g.blocks_per_mcu

        def store(b, k, v):
            blocks[base + b, ZIGZAG[k]] = v
        st = _decode_symbols(sb, luts, g, info.components, 0, 0, 0, sb.end_bit, on_coef=store, stop_blocks=n, counters=counters)
        if st[3] != n or st[4]:
            raise ValueError(f"JPEG: damaged scan ({st[3]} of {n} blocks in {seg}, status {st[4]})")
        if "no_predictor_reset" not in _FAULTS:
            pred = [0, 0, 0]
        for b in range(base, base + n):
            c = 0 if across else g.comp_of[(b - base) % g.blocks_per_mcu]
            pred[c] += int(blocks[b, 0])
            blocks[b, 0] = pred[c]
    if counters is not None:
        counters["segments"] += len(info.segments)
        counters["rst_wrapped"] += int(len(info.segments) > 9)
    return blocks


# ---------------------------------------------------------------------------------------------
# coefficients -> pixels
# ---------------------------------------------------------------------------------------------
def _idct_pass(d, shift):
    """jidctint's one-dimensional pass along the last axis of ``d`` int64 [..., 8]."""
    z2, z3 = d[..., 2], d[..., 6]
    z1 = (z2 + z3) * F["f0_541"]
    t2 = z1 - z3 * F["f1_847"]
    t3 = z1 + z2 * F["f0_765"]
    t0 = (d[..., 0] + d[..., 4]) << 13
    t1 = (d[..., 0] - d[..., 4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = d[..., 7], d[..., 5], d[..., 3], d[..., 1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * F["f1_175"]
    t0, t1, t2, t3 = t0 * F["f0_298"], t1 * F["f2_053"], t2 * F["f3_072"], t3 * F["f1_501"]
    z1, z2, z3, z4 = -z1 * F["f0_899"], -z2 * F["f2_562"], -z3 * F["f1_961"] + z5, -z4 * F["f0_390"] + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    out = np.empty_like(d)
    out[..., 0], out[..., 7] = descale(t10 + t3, shift), descale(t10 - t3, shift)
    out[..., 1], out[..., 6] = descale(t11 + t2, shift), descale(t11 - t2, shift)
    out[..., 2], out[..., 5] = descale(t12 + t1, shift), descale(t12 - t1, shift)
    out[..., 3], out[..., 4] = descale(t13 + t0, shift), descale(t13 - t0, shift)
    return out


def idct_blocks(coefs, qtab):
    """int64 [n, 64] natural order -> samples int64 [n, 8, 8] in 0..255."""
    d = (coefs * qtab[None, :]).reshape(-1, 8, 8)
    d = _idct_pass(d.transpose(0, 2, 1), 11).transpose(0, 2, 1)      # columns
    d = _idct_pass(d, 18)                                             # rows
    return np.clip(d + 128, 0, 255)


def component_planes(info, blocks):
    """The blocks of the scan in coding order -> one plane per component on its block grid."""
    g = info.geometry
    mr, mc, bpm = g.mcu_rows, g.mcus_per_row, g.blocks_per_mcu
    b = blocks.reshape(mr, mc, bpm, 64)
    planes = []
    for c, comp in enumerate(info.components):
        q = info.qtables[comp[3]]
        if c == 0:
            n = g.hs * g.vs
            s = idct_blocks(b[:, :, :n].reshape(-1, 64), q).reshape(mr, mc, g.vs, g.hs, 8, 8)
            planes.append(s.transpose(0, 2, 4, 1, 3, 5).reshape(mr * g.vs * 8, mc * g.hs * 8))
        else:
            s = idct_blocks(b[:, :, g.hs * g.vs + c - 1].reshape(-1, 64), q).reshape(mr, mc, 8, 8)
            planes.append(s.transpose(0, 2, 1, 3).reshape(mr * 8, mc * 8))
    return planes


def _fancy_h(row_sum, dw, bias_even, bias_odd, shift):
    """The horizontal triangle filter on int64 [rows, dw] -> [rows, 2 dw]."""
    last = np.concatenate([row_sum[:, :1], row_sum[:, :-1]], axis=1)
    nxt = np.concatenate([row_sum[:, 1:], row_sum[:, -1:]], axis=1)
    out = np.empty((row_sum.shape[0], 2 * dw), dtype=np.int64)
    out[:, 0::2] = (3 * row_sum + last + bias_even) >> shift
    out[:, 1::2] = (3 * row_sum + nxt + bias_odd) >> shift
    return out


def upsample(plane, g, counters=None):
    """A chroma plane on its block grid -> [H, W] at full resolution, by libjpeg-turbo's rules for this geometry."""
    if g.hs == 1:
        return plane[:g.H, :g.W]
    dw, dh = g.dw, g.dh
    c = plane[:dh, :dw]
    if dw <= 2 and "fancy_narrow" not in _FAULTS:
        if counters is not None:
            counters["narrow_chroma"] += 1
        return np.repeat(np.repeat(c, g.vs, axis=0), 2, axis=1)[:g.H, :g.W]
    b_even, b_odd = (7, 8) if "bias_swapped" in _FAULTS else (8, 7)
    if g.vs == 2:
        above = np.concatenate([c[:1], c[:-1]])
        below = np.concatenate([c[1:], c[-1:]])
        if "far_row_top" in _FAULTS:
            above = np.concatenate([c[1:2] if dh > 1 else c[:1], c[:-1]])
        rows = np.empty((2 * dh, dw), dtype=np.int64)
        rows[0::2], rows[1::2] = 3 * c + above, 3 * c + below
        if counters is not None:
            counters["top_context"] += 1
            counters["bottom_context"] += int(g.H > 2 * dh - 1)
        out = _fancy_h(rows, dw, b_even, b_odd, 4)
    else:
        out = _fancy_h(c, dw, 1, 2, 2)
        out[:, 0], out[:, 2 * dw - 1] = c[:, 0], c[:, dw - 1]
    return out[:g.H, :g.W]


def ycc_to_rgb(y, cb, cr):
    fx = (lambda x: int(x * 65536)) if "fix_floor" in _FAULTS else fix
    cb, cr = cb - 128, cr - 128
    r = y + ((fx(1.402) * cr + 32768) >> 16)
    b = y + ((fx(1.772) * cb + 32768) >> 16)
    gr = y + ((-fx(0.34414) * cb + 32768 - fx(0.71414) * cr) >> 16)
    return np.clip(np.stack([r, gr, b], axis=-1), 0, 255).astype(np.uint8)


def decode_reference(data, counters=None):
    """The pixels of a baseline JPEG file: uint8 [H, W] (one component) or [H, W, 3], equal to np.asarray(Image.open(f)).
    ``counters``: a dict of ``COUNTERS`` that the paths taken are added to."""
    info = data if isinstance(data, Info) else parse(data)
    g = info.geometry
    planes = component_planes(info, scan_coefficients(info, counters))
    if counters is not None:
        counters["odd_h"] += g.H & 1
        counters["odd_w"] += g.W & 1
    y = planes[0][:g.H, :g.W]
    if g.ncomp == 1:
        return y.astype(np.uint8)
    return ycc_to_rgb(y, upsample(planes[1], g, counters), upsample(planes[2], g))


# ---------------------------------------------------------------------------------------------
# the device path
# ---------------------------------------------------------------------------------------------
def device_tables(info):
    """The per-file table block csrc/jpeg_decode.hip reads, int32 [TABLE_WORDS]: the quantisation table of every component
    [3][64] (natural order), the DC and AC table slot of every component [3] + [3] (+ 2 unused), and the four Huffman tables
    DC 0, DC 1, AC 0, AC 1 as limit [16], offset [16], values [256] (``huffman_decode_table``)."""
    t = np.zeros(TABLE_WORDS, dtype=np.int64)
    for c, comp in enumerate(info.components):
        t[64 * c:64 * c + 64] = info.qtables[comp[3]]
        t[192 + c], t[195 + c] = comp[4], comp[5]
    for (cls, tid), spec in info.huffman.items():
        base = 200 + 288 * (2 * cls + tid)
        limit, offset, values = huffman_decode_table(spec)
        t[base:base + 16], t[base + 16:base + 32], t[base + 32:base + 288] = limit, offset, values
    return t.astype(np.int32)


def _read(f):
    if isinstance(f, (bytes, bytearray, memoryview)):
        return bytes(f), "<bytes>"
    with open(f, "rb") as fh:
        return fh.read(), os.fspath(f)


class JpegDecoder:
    """Baseline JPEG files -> uint8 device frames, decoded on the device (csrc/jpeg_decode.hip), equal to
    ``decode_reference`` pixel for pixel.

        dec = JpegDecoder.for_file(device, data)                 # or JpegDecoder(device, height, width, mode)
        frames = dec.decode(files)                               # list of bytes or paths -> [N,H,W,C] (synchronises)
        dec.submit(files_k); ...; frames = dec.collect()         # pipelined: collect() hands back the submission before
        for frame in dec.frames(paths): ...                      # [H,W,C] frames, one chunk decoding ahead

    All files of a decoder share height, width and ``mode`` (one of ``MODES``); their tables, restart intervals and sizes
    may differ.  ``channels=3`` with mode L replicates the channel (``Image.convert("RGB")``).  ``submit`` parses the
    headers on the host, uploads scan bytes, segment records and tables in ONE pinned copy, queues three launches, the copy
    of the N status words into pinned memory and an event on the current stream, and returns; it never waits.  Two
    submissions may be in flight."""

    def __init__(self, device, height, width, mode, channels=None, sub_bytes=DEFAULT_SUB_BYTES):
        import torch
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("JpegDecoder runs on an AMD GPU only (decode_reference is the host definition)")
        self.geometry = Geometry(height, width, mode)
        self.H, self.W, self.mode_name, self.mode = int(height), int(width), mode, MODES.index(mode)
        self.C = int(channels) if channels is not None else (1 if mode == "L" else 3)
        if self.C not in (1, 3) or (mode != "L" and self.C != 3):
            raise ValueError(f"JpegDecoder: channels {channels} does not fit mode {mode!r}")
        if int(sub_bytes) < 1:
            raise ValueError("JpegDecoder: sub_bytes >= 1")
        self.sub_bytes = int(sub_bytes)
        self._slots = [None, None]      # per slot: [pinned staging, device staging, pinned status]
        self._ws = None
        self._pending = InFlight("JpegDecoder")         # remembers (names, out); len(): the submissions not collected yet
        self._last_ws, self._last_shape = None, None      # of the last decode_into (rounds())

    @classmethod
    def for_file(cls, device, data, channels=None, **kw):
        info = parse(_read(data)[0])
        return cls(device, info.H, info.W, info.mode, channels=channels, **kw)

    # ---- host side: files -> one staging block ---------------------------------------------------------------------
    def prepare(self, files, strict=True):
        """Files (bytes, paths or parsed ``Info``) -> (infos, names); a file the decoder does not support or whose geometry
        differs from the decoder's raises here, naming it, before any launch."""
        infos, names = [], []
        for f in files:
            if isinstance(f, Info):                     # a parsed file (tests hand in damaged ones)
                data, name = f.data, "<parsed file>"
            else:
                data, name = _read(f)
            try:
                info = f if isinstance(f, Info) else parse(data, strict=strict)
            except NotImplementedError as e:
                raise NotImplementedError(f"{name}: {e}") from None
            except ValueError as e:
                raise ValueError(f"{name}: {e}") from None
            if (info.H, info.W, info.mode) != (self.H, self.W, self.mode_name):
                raise ValueError(f"{name}: a {info.H}x{info.W} {info.mode} file, the decoder is {self.H}x{self.W} {self.mode_name}")
            infos.append(info)
            names.append(name)
        if not infos:
            raise ValueError("JpegDecoder: no files")
        return infos, names

    @staticmethod
    def pack(infos, skew=0):
        """The staging block of a call, uint8 numpy: tables int32 [N][TABLE_WORDS], segment records int32
        [N][n_segments][4] (begin, end relative to the file's scan bytes, first MCU, MCUs; unused records are zero),
        offsets int32 [N+1], then the scan bytes of all files (``skew`` bytes further on).
        -> (block, n_segments, (tables, segments, offsets, scan) byte offsets)."""
        n = len(infos)
        n_seg = max(len(i.segments) for i in infos)
        tables = np.stack([device_tables(i) for i in infos])
        segs = np.zeros((n, n_seg, 4), dtype=np.int32)
        offsets = np.zeros(n + 1, dtype=np.int32)
        for k, info in enumerate(infos):
            s0 = info.scan[0]
            for j, s in enumerate(info.segments):
                segs[k, j] = (s.begin - s0, s.end - s0, s.first_mcu, s.n_mcus)
            offsets[k + 1] = offsets[k] + (info.scan[1] - s0)
        o_tab, o_seg = 0, tables.nbytes
        o_off = o_seg + segs.nbytes
        o_scan = (o_off + offsets.nbytes + 15) // 16 * 16 + skew
        block = np.zeros(o_scan + int(offsets[-1]) + 16, dtype=np.uint8)
        block[o_tab:o_seg] = tables.view(np.uint8).ravel()
        block[o_seg:o_off] = segs.view(np.uint8).ravel()
        block[o_off:o_off + offsets.nbytes] = offsets.view(np.uint8)
        for k, info in enumerate(infos):
            block[o_scan + offsets[k]:o_scan + offsets[k + 1]] = np.frombuffer(info.data, dtype=np.uint8)[info.scan[0]:info.scan[1]]
        return block, n_seg, (o_tab, o_seg, o_off, o_scan)

    def workspace_bytes(self, n, n_segments):
        from . import _lib
        return _lib.query("ir2rgb_jpeg_decode_workspace_bytes", n, self.H, self.W, self.mode, n_segments)

    def decode_into(self, staged, n, n_segments, layout, out, status, workspace=None, sub_bytes=None):
        """The launches alone, on the current stream: ``staged`` the device copy of ``pack``'s block -> pixels in ``out``
        uint8 [N,H,W,C] and the error bits of every file in ``status`` int32 [N]."""
        import torch
        from . import _lib
        o_tab, o_seg, o_off, o_scan = layout
        if workspace is None:
            need = self.workspace_bytes(n, n_segments)
            if self._ws is None or self._ws.numel() < need:
                self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            workspace = self._ws
        self._last_ws, self._last_shape = workspace, (n, n_segments)
        _lib.launch("ir2rgb_jpeg_decode_u8", out, staged[o_scan:], staged[o_off:], staged[o_seg:], staged[o_tab:], out, status,
                    workspace, workspace.numel(), n, out.shape[3], self.H, self.W, self.mode, n_segments,
                    self.sub_bytes if sub_bytes is None else sub_bytes)

    def rounds(self):
        """Relaxation rounds of every (file, segment) of the last finished call, int32 [N, n_segments] (synchronises)."""
        if self._last_shape is None:
            raise RuntimeError("JpegDecoder.rounds: nothing was decoded")
        n, n_seg = self._last_shape
        off = self.workspace_bytes(n, n_seg) - 8 * n * n_seg
        rec = self._last_ws[off:off + 8 * n * n_seg].cpu().numpy().view(np.int32).reshape(n, n_seg, 2)
        return rec[:, :, 1].copy()

    def submit(self, files, strict=True):
        import torch
        slot = self._pending.slot()
        infos, names = self.prepare(files, strict=strict)
        block, n_seg, layout = self.pack(infos)
        n = len(infos)
        s = self._slots[slot]
        if s is None or s[0].numel() < block.size or s[2].numel() < n:
            size = max(block.size, 2 * s[0].numel() if s else 0)
            s = self._slots[slot] = [torch.empty(size, dtype=torch.uint8, pin_memory=True),
                                     torch.empty(size, dtype=torch.uint8, device=self.device),
                                     torch.empty(max(n, 16), dtype=torch.int32, pin_memory=True)]
        s[0][:block.size].copy_(torch.from_numpy(block))
        out = torch.empty((n, self.H, self.W, self.C), dtype=torch.uint8, device=self.device)
        status = torch.empty(n, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            s[1][:block.size].copy_(s[0][:block.size], non_blocking=True)
            self.decode_into(s[1], n, n_seg, layout, out, status)
            s[2][:n].copy_(status, non_blocking=True)
            self._pending.push(names, out)

    def collect(self):
        """The frames of the oldest submission in flight, uint8 [N,H,W,C] on the device."""
        slot, names, out = self._pending.pop()
        status = self._slots[slot][2][:len(names)].tolist()
        for name, st in zip(names, status):
            if st:
                what = ", ".join(v for b, v in ERR_NAMES.items() if st & b)
                raise ValueError(f"{name}: damaged JPEG scan (status {st:#x}: {what})")
        return out

    def decode(self, files):
        self._pending.require_idle("decode")
        self.submit(files)
        return self.collect()

    def frames(self, files, chunk=16):
        """Generator over uint8 [H,W,C] device frames of ``files`` in order; the next chunk of ``chunk`` files is parsed,
        uploaded and decoding while the frames of this one are consumed."""
        files = list(files)
        self._pending.require_idle("frames")
        chunks = [files[i:i + chunk] for i in range(0, len(files), int(chunk))]
        if chunks:
            self.submit(chunks[0])
        for i in range(len(chunks)):
            if i + 1 < len(chunks):
                self.submit(chunks[i + 1])
            yield from self.collect()
