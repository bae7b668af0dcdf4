// jpeg.hip -- baseline JPEG files of uint8 frames that stay on the device, equal byte for byte to the files Pillow (libjpeg)
// writes: Image.save(f, "JPEG", quality=q, subsampling=..., restart_marker_rows=r).  The definition, rule by rule in
// libjpeg's statement order, is ir2rgb_amd/jpeg.py (jpeg_reference); everything here is integer arithmetic.
//
// A file is the header the host built (SOI .. SOS, uploaded once) followed by the scan.  The unit of parallelism is the
// restart interval (restart_rows MCU rows): DC prediction restarts there and every interval ends on a byte boundary, so
// intervals are coded independently and only their byte counts chain.  Three launches, whatever N and the pixels are:
//
//   jpeg_blocks_kernel    one thread per 8x8 block of the scan, in coding order: colour conversion (jccolor), h2v2
//                         downsampling with libjpeg's edge rules, jfdctint, quantisation, the dummy-block rule
//                         -> int16 [N][blocks][64] in zigzag order.  A dummy block recomputes the block its DC comes from.
//   jpeg_entropy_kernel   one workgroup per (interval, frame).  The interval is taken in chunks of 128 blocks, one per
//                         thread: bit length of every block, a fixed-order scan, the codes or-ed into an LDS bit buffer at
//                         their offsets, then byte stuffing into the interval's scratch region.  LDS holds the worst case of
//                         ONE CHUNK (53 words per block >= 27 + 63 * 26 bits), never of an interval; the bits that do not
//                         fill a byte are carried into the next chunk.  -> scratch bytes and the interval's byte count.
//   jpeg_pack_kernel      one workgroup per (interval, frame): the sum of the byte counts before it places the interval
//                         behind the header; it appends FF D0+(i mod 8), or FF D9 after the last one, which also writes the
//                         file's length; the first one copies the header.
//
// Bounds.  Code lengths read from the caller's tables are clamped to max_dc / max_ac and size categories to 11 / 10, so a
// block codes to at most  blk_bits = (max_dc + 11) + 63 * (max_ac + 10)  bits whatever the tables and pixels hold: the DC
// code, and at most 63 AC codes, because every AC code (a coefficient, ZRL, EOB) accounts for at least one of the 63
// positions that no other code accounts for.  An interval of B blocks is therefore at most ceil(B * blk_bits / 8) bytes
// with its padding and twice that after stuffing: the size of its scratch region and, plus two marker bytes per interval
// and the header, ir2rgb_jpeg_capacity_bytes.  Sample coordinates are clamped to the frame, table indices to the tables.
#include "jpeg_common.h"    // shared with jpeg_decode.hip: modes, ZZ, DCT multipliers, descale, scan_inclusive, align16, jpeg_grid
#include "u8.h"             // the bytes of a dword

namespace {

constexpr int TAB_DC = 128, TAB_AC = 160, TAB_WORDS = IR2RGB_JPEG_TABLE_WORDS;      // quantisation [2][64], DC [2][16], AC [2][256]
constexpr int ENT_THREADS = 128;                                    // blocks per chunk of the entropy kernel
constexpr int BLK_WORDS = 53;                                       // LDS words per block: 1696 bits >= 27 + 63 * 26
constexpr int BUF_WORDS = ENT_THREADS * BLK_WORDS + 2;
constexpr int PACK_THREADS = 256;

struct Geom : JpegGrid {
    int wib, hib;               // real luminance blocks per row / column
    int rows_per_int, n_int;    // MCU rows per restart interval, intervals per frame
    int max_dc, max_ac;
    int header_bytes;
    long int_cap;               // scratch bytes per interval
};

// ---- samples ----------------------------------------------------------------------------------------------------------
// jccolor with 16 fraction bits, FIX(x) = int(x * 65536 + 0.5)
__device__ __forceinline__ int ycc(const uint8_t *p, int comp) {
    const int r = p[0], g = p[1], b = p[2];
    if (comp == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    if (comp == 1) return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
    return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

__device__ __forceinline__ const uint8_t *pixel(const uint8_t *f, const Geom &g, int y, int x) {
    return f + ((long)min(y, g.H - 1) * g.W + min(x, g.W - 1)) * g.C;
}

// sample (y, x) of a component on its own grid, edges replicated
template <int MODE> __device__ __forceinline__ int sample(const uint8_t *f, const Geom &g, int comp, int y, int x) {
    if (MODE == MODE_L) return pixel(f, g, y, x)[0];
    if (MODE == MODE_444 || comp == 0) return ycc(pixel(f, g, y, x), comp);
    // h2v2: the full-resolution plane is extended first (clamped coordinates), the bias alternates 1, 2 by OUTPUT column,
    // padded columns included; rows below the last chroma row repeat it
    y = min(y, (g.H + 1) / 2 - 1);
    const int bias = 1 + (x & 1);
    return (ycc(pixel(f, g, 2 * y, 2 * x), comp) + ycc(pixel(f, g, 2 * y, 2 * x + 1), comp) +
            ycc(pixel(f, g, 2 * y + 1, 2 * x), comp) + ycc(pixel(f, g, 2 * y + 1, 2 * x + 1), comp) + bias) >> 2;
}

// ---- jfdctint -----------------------------------------------------------------------------------------------------------
// one pass over 8 values d[0], d[S], ... d[7 S]; FIRST: rows (results scaled by 4), else columns
template <int S, bool FIRST> __device__ __forceinline__ void fdct8(int *d) {
    constexpr int N = FIRST ? 13 - 2 : 13 + 2;
    int t0 = d[0] + d[7 * S], t7 = d[0] - d[7 * S], t1 = d[S] + d[6 * S], t6 = d[S] - d[6 * S];
    int t2 = d[2 * S] + d[5 * S], t5 = d[2 * S] - d[5 * S], t3 = d[3 * S] + d[4 * S], t4 = d[3 * S] - d[4 * S];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    d[0] = FIRST ? (t10 + t11) << 2 : descale(t10 + t11, 2);
    d[4 * S] = FIRST ? (t10 - t11) << 2 : descale(t10 - t11, 2);
    int z1 = (t12 + t13) * F0_541;
    d[2 * S] = descale(z1 + t13 * F0_765, N);
    d[6 * S] = descale(z1 - t12 * F1_847, N);
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * F1_175;
    t4 *= F0_298, t5 *= F2_053, t6 *= F3_072, t7 *= F1_501;
    z1 *= -F0_899, z2 *= -F2_562, z3 = z3 * -F1_961 + z5, z4 = z4 * -F0_390 + z5;
    d[7 * S] = descale(t4 + z1 + z3, N);
    d[5 * S] = descale(t5 + z2 + z4, N);
    d[3 * S] = descale(t6 + z2 + z3, N);
    d[S] = descale(t7 + z1 + z4, N);
}

template <int MODE>
__global__ void __launch_bounds__(64)
jpeg_blocks_kernel(const uint8_t *__restrict__ src, uint4 *__restrict__ coefs, const unsigned *__restrict__ tables, Geom g,
                   int total) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= total) return;
    const int n = i / g.nblk, b = i % g.nblk;
    const int mcu = b / g.bpm, k = b % g.bpm;
    const int mr = mcu / g.mcus_per_row, mc = mcu % g.mcus_per_row;
    const uint8_t *f = src + (long)n * g.H * g.W * g.C;
    int comp = 0, by = mr, bx = mc;
    bool dummy = false;
    if (MODE == MODE_444) comp = k;
    if (MODE == MODE_420) {
        if (k < 4) {
            by = 2 * mr + (k >> 1), bx = 2 * mc + (k & 1);
            // the block a dummy block takes its DC from: the last block of the MCU's first row, then the one before it
            if (by >= g.hib) dummy = true, by = 2 * mr, bx = 2 * mc + 1;
            if (bx >= g.wib) dummy = true, bx = 2 * mc;
        } else {
            comp = k - 3;
        }
    }
    int d[64];
#pragma unroll
    for (int y = 0; y < 8; ++y)
#pragma unroll
        for (int x = 0; x < 8; ++x) d[8 * y + x] = sample<MODE>(f, g, comp, 8 * by + y, 8 * bx + x) - 128;
#pragma unroll
    for (int r = 0; r < 8; ++r) fdct8<1, true>(d + 8 * r);
#pragma unroll
    for (int c = 0; c < 8; ++c) fdct8<8, false>(d + c);
    const unsigned *q = tables + (comp ? 64 : 0);
    unsigned w[32] = {};
#pragma unroll
    for (int z = 0; z < 64; ++z) {
        const int c = d[ZZ[z]];
        const int div = (int)min(max(q[ZZ[z]], 1u), 255u) << 3;
        const int m = (abs(c) + (div >> 1)) / div;
        const int v = (dummy && z) ? 0 : (c < 0 ? -m : m);
        w[z >> 1] |= ((unsigned)v & 0xffffu) << (16 * (z & 1));
    }
    uint4 *out = coefs + (long)i * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) out[j] = make_uint4(w[4 * j], w[4 * j + 1], w[4 * j + 2], w[4 * j + 3]);
}

// ---- entropy coding -----------------------------------------------------------------------------------------------------
// nb (1..27) low bits of v into the big-endian bit stream buf at bit position pos
__device__ __forceinline__ void put_bits(unsigned *buf, int pos, unsigned v, int nb) {
    const int w = pos >> 5, room = 32 - (pos & 31);
    if (nb <= room) {
        atomicOr(&buf[w], v << (room - nb));
    } else {
        atomicOr(&buf[w], v >> (nb - room));
        atomicOr(&buf[w + 1], v << (32 - (nb - room)));
    }
}

__device__ __forceinline__ unsigned stream_byte(const unsigned *buf, int j) { return get_byte(buf[j >> 2], 3 - (j & 3)); }

// the code of a (table entry, value of size category s) pair: (code << s | value bits), its length in *nb
__device__ __forceinline__ unsigned code_of(unsigned entry, int max_len, int v, int s, int *nb) {
    const int len = min((int)(entry >> 16), max_len);
    const unsigned code = entry & ((1u << len) - 1u);
    *nb = len + s;
    return (code << s) | ((unsigned)(v < 0 ? v - 1 : v) & ((1u << s) - 1u));
}

// one block at bit position pos of buf (EMIT) or nowhere -> the position after it.  dc / ac: this component's tables (LDS)
template <bool EMIT>
__device__ int encode_block(const int16_t *__restrict__ blk, int pred, const unsigned *dc, const unsigned *ac, int max_dc,
                            int max_ac, unsigned *buf, int pos) {
    int nb;
    const int diff = (int)blk[0] - pred;
    int s = min(32 - __clz(abs(diff)), 11);
    unsigned v = code_of(dc[s], max_dc, diff, s, &nb);
    if (EMIT && nb) put_bits(buf, pos, v, nb);
    pos += nb;
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        const int c = blk[k];
        if (c == 0) {
            ++run;
            continue;
        }
        for (; run > 15; run -= 16) {
            v = code_of(ac[0xF0], max_ac, 0, 0, &nb);
            if (EMIT && nb) put_bits(buf, pos, v, nb);
            pos += nb;
        }
        s = min(32 - __clz(abs(c)), 10);
        v = code_of(ac[(run << 4) | s], max_ac, c, s, &nb);
        if (EMIT && nb) put_bits(buf, pos, v, nb);
        pos += nb;
        run = 0;
    }
    if (run) {
        v = code_of(ac[0], max_ac, 0, 0, &nb);
        if (EMIT && nb) put_bits(buf, pos, v, nb);
        pos += nb;
    }
    return pos;
}

__global__ void __launch_bounds__(ENT_THREADS)
jpeg_entropy_kernel(const int16_t *__restrict__ coefs, const unsigned *__restrict__ tables, uint8_t *__restrict__ scratch,
                    int *__restrict__ int_len, Geom g) {
    __shared__ unsigned tab[TAB_WORDS - TAB_DC];
    __shared__ unsigned buf[BUF_WORDS];
    __shared__ int sh[ENT_THREADS];
    const int t = threadIdx.x, it = blockIdx.x, n = blockIdx.y;
    for (int i = t; i < TAB_WORDS - TAB_DC; i += ENT_THREADS) tab[i] = tables[TAB_DC + i];
    __syncthreads();
    const int per_row = g.mcus_per_row * g.bpm;
    const int nb_int = min(g.rows_per_int, g.mcu_rows - it * g.rows_per_int) * per_row;        // blocks of this interval
    const int16_t *cf = coefs + ((long)n * g.nblk + (long)it * g.rows_per_int * per_row) * 64;
    uint8_t *dst = scratch + ((long)n * g.n_int + it) * g.int_cap;
    int carry_bits = 0, out_pos = 0;
    unsigned carry_val = 0;             // the carry_bits bits that did not fill a byte, in the high bits of a byte
    for (int base = 0; base < nb_int; base += ENT_THREADS) {
        const int j = base + t;
        const bool live = j < nb_int, last = base + ENT_THREADS >= nb_int;
        // the block this one's DC is predicted from: the previous block of its component inside the interval
        const int k = j % g.bpm, first_mcu = j < g.bpm;
        int prev, chroma;
        if (g.mode == MODE_420) {
            chroma = k >= 4;
            prev = (k >= 1 && k <= 3) ? j - 1 : (first_mcu ? -1 : (k == 0 ? j - 3 : j - 6));
        } else {
            chroma = k > 0;
            prev = first_mcu ? -1 : j - g.bpm;
        }
        const int pred = (live && prev >= 0) ? cf[(long)prev * 64] : 0;
        const unsigned *dc = tab + 16 * chroma, *ac = tab + (TAB_AC - TAB_DC) + 256 * chroma;
        const int16_t *blk = cf + (long)j * 64;
        const int len = live ? encode_block<false>(blk, pred, dc, ac, g.max_dc, g.max_ac, nullptr, 0) : 0;
        int sum;
        const int end = scan_inclusive<ENT_THREADS>(len, sh, &sum);
        const int total = carry_bits + sum;
        const int words = (total + 31) / 32 + 1;
        for (int w = t; w < words; w += ENT_THREADS) buf[w] = w == 0 ? carry_val << 24 : 0u;
        __syncthreads();
        if (live) encode_block<true>(blk, pred, dc, ac, g.max_dc, g.max_ac, buf, carry_bits + end - len);
        const int pad = last ? (8 - (total & 7)) & 7 : 0;               // the interval ends on a byte boundary: 1-bits
        if (t == 0 && pad) put_bits(buf, total, (1u << pad) - 1u, pad);
        __syncthreads();
        const int nbytes = (total + pad) / 8;
        // stuffing: every thread takes a run of consecutive bytes; 0x00 follows every 0xFF
        const int per = (nbytes + ENT_THREADS - 1) / ENT_THREADS;
        const int lo = min(t * per, nbytes), hi = min(lo + per, nbytes);
        int ff = 0;
        for (int b = lo; b < hi; ++b) ff += stream_byte(buf, b) == 0xffu;
        int all_ff;
        const int ff_end = scan_inclusive<ENT_THREADS>(ff, sh, &all_ff);
        uint8_t *o = dst + out_pos + lo + (ff_end - ff);
        for (int b = lo; b < hi; ++b) {
            const unsigned v = stream_byte(buf, b);
            *o++ = (uint8_t)v;
            if (v == 0xffu) *o++ = 0;
        }
        carry_bits = (total + pad) & 7;
        carry_val = carry_bits ? stream_byte(buf, nbytes) : 0u;
        out_pos += nbytes + all_ff;
    }
    if (t == 0) int_len[n * g.n_int + it] = out_pos;
}

__global__ void __launch_bounds__(PACK_THREADS)
jpeg_pack_kernel(const uint8_t *__restrict__ scratch, const int *__restrict__ int_len, const uint8_t *__restrict__ header,
                 uint8_t *__restrict__ out, int *__restrict__ lengths, long capacity, Geom g) {
    __shared__ int before;
    const int t = threadIdx.x, it = blockIdx.x, n = blockIdx.y;
    const int *len = int_len + n * g.n_int;
    if (t == 0) before = 0;
    __syncthreads();
    int part = 0;
    for (int j = t; j < it; j += PACK_THREADS) part += len[j] + 2;
    if (part) atomicAdd(&before, part);
    __syncthreads();
    uint8_t *file = out + (long)n * capacity;
    const int off = g.header_bytes + before, mine = len[it];
    const uint8_t *src = scratch + ((long)n * g.n_int + it) * g.int_cap;
    for (int b = t; b < mine; b += PACK_THREADS) file[off + b] = src[b];
    const bool last = it == g.n_int - 1;
    if (t == 0) {
        file[off + mine] = 0xff;
        file[off + mine + 1] = (uint8_t)(last ? 0xd9 : 0xd0 + (it & 7));
        if (last) lengths[n] = off + mine + 2;
    }
    if (it == 0)
        for (int b = t; b < g.header_bytes; b += PACK_THREADS) file[b] = header[b];
}

// ---- host ---------------------------------------------------------------------------------------------------------------
// IR2RGB_OK and the geometry, or IR2RGB_EINVAL.  4:2:2 is read (jpeg_decode.hip), not written.
int geometry(int N, int C, int H, int W, int mode, int restart_rows, int max_dc, int max_ac, int header_bytes, Geom *g) {
    if (mode == MODE_422 || restart_rows < 1 || jpeg_grid(N, C, H, W, mode, g) != IR2RGB_OK) return IR2RGB_EINVAL;
    if (max_dc < 1 || max_dc > 16 || max_ac < 1 || max_ac > 16 || header_bytes < 0 || header_bytes > 65535) return IR2RGB_EINVAL;
    g->wib = (W + 7) / 8, g->hib = (H + 7) / 8;
    if ((long)restart_rows * g->mcus_per_row > 65535) return IR2RGB_EINVAL;        // the DRI field
    g->rows_per_int = restart_rows < g->mcu_rows ? restart_rows : g->mcu_rows;
    g->n_int = (g->mcu_rows + g->rows_per_int - 1) / g->rows_per_int;
    g->max_dc = max_dc, g->max_ac = max_ac, g->header_bytes = header_bytes;
    const long blk_bits = (max_dc + 11) + 63L * (max_ac + 10);
    const long int_blocks = (long)g->rows_per_int * g->mcus_per_row * g->bpm;
    g->int_cap = align16(2 * ((int_blocks * blk_bits + 7) / 8));
    if (header_bytes + (long)g->n_int * (g->int_cap + 2) > 0x7fffffffL) return IR2RGB_EINVAL;      // a file is addressed in int
    return IR2RGB_OK;
}

long capacity_of(const Geom &g) { return g.header_bytes + (long)g.n_int * (g.int_cap + 2); }

struct Workspace {
    long coefs, lens, scratch, bytes;       // byte offsets of the three regions, and the size
};
Workspace workspace_of(const Geom &g, int N) {
    Workspace w;
    w.coefs = 0;
    w.lens = (long)N * g.nblk * 128;
    w.scratch = w.lens + align16((long)N * g.n_int * 4);
    w.bytes = w.scratch + (long)N * g.n_int * g.int_cap;
    return w;
}

}  // namespace

extern "C" long ir2rgb_jpeg_workspace_bytes(int N, int H, int W, int mode, int restart_rows, int max_dc_len, int max_ac_len) {
    Geom g;
    const int rc = geometry(N, mode == MODE_L ? 1 : 3, H, W, mode, restart_rows, max_dc_len, max_ac_len, 0, &g);
    if (rc != IR2RGB_OK) return rc;
    return workspace_of(g, N).bytes;
}

extern "C" long ir2rgb_jpeg_capacity_bytes(int H, int W, int mode, int restart_rows, int header_bytes, int max_dc_len,
                                           int max_ac_len) {
    Geom g;
    const int rc = geometry(1, mode == MODE_L ? 1 : 3, H, W, mode, restart_rows, max_dc_len, max_ac_len, header_bytes, &g);
    if (rc != IR2RGB_OK) return rc;
    return capacity_of(g);
}

extern "C" int ir2rgb_jpeg_encode_u8(const uint8_t *src, uint8_t *out, int *lengths, void *workspace, long workspace_bytes,
                                     const uint8_t *header, int header_bytes, const unsigned *tables, int N, int C, int H, int W,
                                     int mode, int restart_rows, int max_dc_len, int max_ac_len, long capacity, void *stream) {
    Geom g;
    const int rc = geometry(N, C, H, W, mode, restart_rows, max_dc_len, max_ac_len, header_bytes, &g);
    if (rc != IR2RGB_OK) return rc;
    if (!src || !out || !lengths || !workspace || !header || !tables || header_bytes < 1) return IR2RGB_EINVAL;
    const Workspace ws = workspace_of(g, N);
    if (workspace_bytes < ws.bytes || capacity < capacity_of(g)) return IR2RGB_EINVAL;
    if (misaligned(workspace, 16) || misaligned(tables, 4) || misaligned(lengths, 4)) return IR2RGB_EALIGN;
    hipStream_t s = as_stream(stream);
    uint8_t *base = static_cast<uint8_t *>(workspace);
    uint4 *coefs = reinterpret_cast<uint4 *>(base + ws.coefs);
    int *int_len = reinterpret_cast<int *>(base + ws.lens);
    uint8_t *scratch = base + ws.scratch;
    const int total = N * g.nblk;
    if (mode == MODE_420) jpeg_blocks_kernel<MODE_420><<<cdiv(total, 64), 64, 0, s>>>(src, coefs, tables, g, total);
    else if (mode == MODE_444) jpeg_blocks_kernel<MODE_444><<<cdiv(total, 64), 64, 0, s>>>(src, coefs, tables, g, total);
    else jpeg_blocks_kernel<MODE_L><<<cdiv(total, 64), 64, 0, s>>>(src, coefs, tables, g, total);
    const dim3 grid(g.n_int, N);
    jpeg_entropy_kernel<<<grid, ENT_THREADS, 0, s>>>(reinterpret_cast<const int16_t *>(coefs), tables, scratch, int_len, g);
    jpeg_pack_kernel<<<grid, PACK_THREADS, 0, s>>>(scratch, int_len, header, out, lengths, capacity, g);
    return ir2rgb_launch_status();
}
