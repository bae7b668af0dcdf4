// jpeg_decode.hip -- baseline JPEG files decoded on the device into uint8 frames, equal pixel for pixel to what Pillow
// (libjpeg-turbo) decodes: np.asarray(Image.open(f)).  The definition, rule by rule, is ir2rgb_amd/jpeg_decode.py
// (decode_reference for the pixels, entropy_model for the parallel entropy decode); everything here is integer arithmetic.
//
// Camera files usually carry no restart markers, so the restart interval (a "segment") cannot be the only unit of
// parallelism.  Inside a segment the raw, still-stuffed bytes are cut into subsequences of sub_bytes, one thread each, and
// the threads relax towards the sequential decoder's states -- Huffman streams resynchronise after a wrong entry:
//
//   jpegd_entropy_kernel  one workgroup per (segment, file).  A state between two symbols is (raw bit position, block
//                         within the MCU, zigzag position k).  Subsequence 0 enters at (0, 0, 0), the others at a guess
//                         (their first byte, block 0, k 0).  A round: every thread whose entry changed decodes, without
//                         storing, the symbols that start inside its subsequence; its exit state is its right neighbour's
//                         next entry.  After round r entries 0..r are true, so the loop is a for over n_sub rounds that
//                         a round without a change leaves early.  Then a scan of the completed-block counts gives every
//                         thread its first output block, the segment's blocks are zeroed behind a barrier (a block may
//                         span threads), a write pass decodes once more and stores the coefficients, and a fixed-order
//                         scan of the DC differences per component turns them into values.
//                         -> int16 [N][blocks][64] in coding order, natural order inside a block.
//   jpegd_idct_kernel     one thread per block: dequantise, jpeg_idct_islow, + 128, clamp -> uint8 component planes on
//                         their block grids.
//   jpegd_pixels_kernel   one thread per pixel: libjpeg-turbo's upsampling for the geometry (replication when the chroma
//                         plane is at most 2 wide, else the h2v2 / h2v1 triangle filters), jdcolor -> [N][H][W][C]; its
//                         first workgroup per file folds the segments' error bits into status[n].
//
// Bounds.  A wrong-sync decode reads garbage codes by design, and a file may hold anything, so nothing below trusts a
// decoded value: a byte is read only inside the segment's range (clamped to the file's; past the end the reader supplies
// 1-bits), every table index is clamped to its table, k never passes 64 (a block ends there), 16 bits that are no code are
// consumed as symbol 0 (so every symbol consumes at least one bit and the loops end), a coefficient is stored only into a
// block of the segment, and segment records are clamped to the frame's MCUs.  Only the write pass reports errors.
#include "jpeg_common.h"    // shared with jpeg.hip: modes, ZZ, DCT multipliers, descale, scan_inclusive, align16, jpeg_grid

namespace {

constexpr int TAB_COMP = 192, TAB_HUFF = 200, HUFF_WORDS = 288, TAB_WORDS = IR2RGB_JPEGD_TABLE_WORDS;
constexpr int ENT_THREADS = IR2RGB_JPEGD_THREADS;
constexpr int PIX_THREADS = 256;

struct DGeom : JpegGrid {
    int ncomp, n_mcus;
    int pw[3], ph[3];           // component planes (block grids)
    long po[3], plane_bytes;    // their byte offsets inside a file's planes, and the size of all
    int dw, dh;                 // real size of the chroma planes
    int n_seg;                  // segment records per file
};

// ---- entropy decoding ---------------------------------------------------------------------------------------------------
// byte i >= 0 of a segment of n bytes; past the end the reader supplies 1-bits
__device__ __forceinline__ unsigned seg_byte(const uint8_t *d, int n, int i) { return i < n ? d[i] : 0xffu; }

// The six data bytes from the byte of bit position p on (p never points into a stuffing byte; a byte is stuffing when it
// is 00 and the raw byte before it is FF).  skips: 4 bits per data byte, the stuffing bytes passed before it.
__device__ __forceinline__ uint64_t window48(const uint8_t *d, int n, int p, unsigned *skips) {
    int idx = p >> 3;
    unsigned prev = (idx > 0 && idx <= n) ? d[idx - 1] : 0u, sk = 0, all = 0;
    uint64_t w = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        unsigned c = seg_byte(d, n, idx);
        if (prev == 0xffu && c == 0u && idx < n) {
            ++sk, ++idx;
            c = seg_byte(d, n, idx);
        }
        w = (w << 8) | c;
        all |= sk << (4 * i);
        prev = c;
        ++idx;
    }
    *skips = all;
    return w;
}

struct Tables {
    const unsigned *huff;       // LDS: four tables of limit [16], offset [16], values [256]
    int dc[3], ac[3];           // table slot of every component
};

// Decodes the symbols that start in [p, end) from the state (p, blk, k).  WRITE: stores coefficients into blocks
// [first_block + done ...) of ``out`` (seg_blocks blocks), stops once seg_blocks are complete, and reports errors.
template <bool WRITE>
__device__ void decode_run(const uint8_t *d, int n, const Tables &T, const DGeom &g, int &p, int &blk, int &k, int end, int &done,
                           int16_t *out, int seg_blocks, int first_block, int &status) {
    const int ny = g.hs * g.vs;
    while (p < end) {
        if (WRITE && first_block + done >= seg_blocks) {
            // more than 7 data bits left (p < end: its byte is inside the segment; stuffing does not count)
            const int idx = p >> 3;
            int next = idx + 1;
            if (next < n && d[idx] == 0xff && d[next] == 0) ++next;
            if (next < n || (p & 7) == 0) status |= IR2RGB_JPEGD_ELEFTOVER;
            break;
        }
        const int comp = blk < ny ? 0 : min(blk - ny + 1, 2);
        const unsigned *tab = T.huff + HUFF_WORDS * (k == 0 ? T.dc[comp] : 2 + T.ac[comp]);
        unsigned skips;
        const int bit = p & 7;
        const uint64_t w = (window48(d, n, p, &skips) << bit) & 0xffffffffffffull;
        const unsigned peek = (unsigned)(w >> 32);
        int len = 1;
        for (; len <= 16; ++len)
            if (peek < tab[len - 1]) break;
        unsigned sym = 0;
        if (len > 16) {
            len = 16;
            if (WRITE) status |= IR2RGB_JPEGD_ECODE;
        } else {
            const int vi = (int)tab[16 + len - 1] + (int)(peek >> (16 - len));
            sym = tab[32 + min(max(vi, 0), 255)] & 0xffu;
        }
        const int s = k == 0 ? min((int)sym, 16) : (int)(sym & 15u), run = k == 0 ? 0 : (int)(sym >> 4);
        int v = s ? (int)(((w << len) & 0xffffffffffffull) >> (48 - s)) : 0;
        if (s && v < (1 << (s - 1))) v = v - (1 << s) + 1;
        const int total = bit + len + s, nb = total >> 3;                  // nb <= 4
        p = ((p >> 3) + nb + (int)((skips >> (4 * nb)) & 15u)) * 8 + (total & 7);
        int at = -1;                                                      // zigzag position of a coefficient to store
        if (k == 0) {
            at = 0, k = 1;
        } else if (s) {
            k += run;
            if (k > 63) {
                if (WRITE) status |= IR2RGB_JPEGD_EINDEX;
                k = 64;
            } else {
                at = k, ++k;
            }
        } else if (run == 15) {
            k += 16;
            if (k > 64) {
                if (WRITE) status |= IR2RGB_JPEGD_EINDEX;
                k = 64;
            }
        } else {
            k = 64;
        }
        if (WRITE && at >= 0) {
            const int b = first_block + done;
            if (b >= 0 && b < seg_blocks) out[(long)b * 64 + ZZ[at & 63]] = (int16_t)v;
        }
        if (k >= 64) {
            k = 0;
            blk = blk + 1 < g.bpm ? blk + 1 : 0;
            ++done;
        }
    }
}

__global__ void __launch_bounds__(ENT_THREADS)
jpegd_entropy_kernel(const uint8_t *__restrict__ files, const int *__restrict__ file_offsets, const int *__restrict__ segments,
                     const int *__restrict__ tables, int16_t *__restrict__ coefs, int *__restrict__ seg_info, DGeom g,
                     int sub_bytes) {
    __shared__ unsigned huff[4 * HUFF_WORDS];
    __shared__ int exit_p[ENT_THREADS], exit_st[ENT_THREADS], sh[ENT_THREADS];
    __shared__ int sh_status;
    const int t = threadIdx.x, seg = blockIdx.x, n = blockIdx.y;
    const int *rec = segments + ((long)n * g.n_seg + seg) * 4;
    const int off0 = file_offsets[n], flen = max(file_offsets[n + 1] - off0, 0);
    const int b0 = min(max(rec[0], 0), flen), b1 = min(max(rec[1], b0), flen);
    int first = rec[2], n_mcus = rec[3], status = 0;
    if (first < 0 || n_mcus < 0 || (long)first + n_mcus > g.n_mcus) {
        status |= IR2RGB_JPEGD_ESEGMENT;
        first = min(max(first, 0), g.n_mcus);
        n_mcus = min(max(n_mcus, 0), g.n_mcus - first);
    }
    int *info = seg_info + ((long)n * g.n_seg + seg) * 2;
    if (n_mcus == 0) {                                  // an unused record (uniform over the workgroup)
        if (t == 0) info[0] = status, info[1] = 0;
        return;
    }
    const int *ftab = tables + (long)n * TAB_WORDS;
    for (int i = t; i < 4 * HUFF_WORDS; i += ENT_THREADS) huff[i] = (unsigned)ftab[TAB_HUFF + i];
    if (t == 0) sh_status = 0;
    Tables T;
    T.huff = huff;
    for (int c = 0; c < 3; ++c) T.dc[c] = ftab[TAB_COMP + c] & 1, T.ac[c] = ftab[TAB_COMP + 3 + c] & 1;
    __syncthreads();

    const uint8_t *d = files + off0 + b0;
    const int len = b1 - b0;
    const int sub = max(max(sub_bytes, (len + ENT_THREADS - 1) / ENT_THREADS), 1);
    const int n_sub = max((len + sub - 1) / sub, 1);                    // <= ENT_THREADS
    const bool active = t < n_sub;
    const int start = min(t * sub, len);
    const int end = active ? (t == n_sub - 1 ? len : start + sub) * 8 : 0;
    // the guess: this subsequence's first data byte, block 0, k 0 (subsequence 0: the true state)
    int entry_p = 8 * start, entry_st = 0;
    if (active && t > 0 && d[start - 1] == 0xff && d[start] == 0) entry_p += 8;
    int count = 0, rounds = 0, dummy = 0;
    bool dirty = active;
    for (int r = 0; r < n_sub; ++r) {
        ++rounds;
        if (dirty) {
            int p = entry_p, blk = entry_st >> 7, k = entry_st & 127;
            count = 0;
            decode_run<false>(d, len, T, g, p, blk, k, end, count, nullptr, 0, 0, dummy);
            exit_p[t] = p, exit_st[t] = (blk << 7) | k;
        }
        __syncthreads();
        dirty = false;
        if (active && t > 0) {
            const int p = exit_p[t - 1], st = exit_st[t - 1];
            if (p != entry_p || st != entry_st) entry_p = p, entry_st = st, dirty = true;
        }
        if (!__syncthreads_or(dirty)) break;
    }
    // the first output block of every subsequence
    const int seg_blocks = n_mcus * g.bpm;
    int total;
    const int before = scan_inclusive<ENT_THREADS>(active ? count : 0, sh, &total) - (active ? count : 0);
    if (t == 0 && total != seg_blocks) status |= IR2RGB_JPEGD_EBLOCKS;
    int16_t *out = coefs + ((long)n * g.nblk + (long)first * g.bpm) * 64;
    uint4 *out4 = reinterpret_cast<uint4 *>(out);
    for (int i = t; i < seg_blocks * 8; i += ENT_THREADS) out4[i] = make_uint4(0, 0, 0, 0);
    __syncthreads();
    if (active) {
        int p = entry_p, blk = entry_st >> 7, k = entry_st & 127, done = 0;
        decode_run<true>(d, len, T, g, p, blk, k, end, done, out, seg_blocks, before, status);
    }
    __syncthreads();
    // DC: differences -> values, per component in coding order; every thread takes a run of consecutive MCUs
    const int per = (n_mcus + ENT_THREADS - 1) / ENT_THREADS;
    const int m0 = min(t * per, n_mcus), m1 = min(m0 + per, n_mcus), ny = g.hs * g.vs;
    int sum[3] = {0, 0, 0};
    for (int m = m0; m < m1; ++m)
        for (int j = 0; j < g.bpm; ++j) sum[j < ny ? 0 : j - ny + 1] += out[((long)m * g.bpm + j) * 64];
    int pred[3];
    for (int c = 0; c < 3; ++c) pred[c] = scan_inclusive<ENT_THREADS>(sum[c], sh, &total) - sum[c];
    for (int m = m0; m < m1; ++m)
        for (int j = 0; j < g.bpm; ++j) {
            const int c = j < ny ? 0 : j - ny + 1;
            int16_t *dc = out + ((long)m * g.bpm + j) * 64;
            pred[c] += *dc;
            *dc = (int16_t)pred[c];
        }
    if (status) atomicOr(&sh_status, status);
    __syncthreads();
    if (t == 0) info[0] = sh_status, info[1] = rounds;
}

// ---- jidctint -------------------------------------------------------------------------------------------------------------
// one pass over 8 values d[0], d[S], ... d[7 S]
template <int S, int SHIFT> __device__ __forceinline__ void idct8(int *d) {
    int z2 = d[2 * S], z3 = d[6 * S];
    int z1 = (z2 + z3) * F0_541;
    int t2 = z1 - z3 * F1_847, t3 = z1 + z2 * F0_765;
    int t0 = (d[0] + d[4 * S]) << 13, t1 = (d[0] - d[4 * S]) << 13;
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    t0 = d[7 * S], t1 = d[5 * S], t2 = d[3 * S], t3 = d[S];
    z1 = t0 + t3, z2 = t1 + t2, z3 = t0 + t2;
    int z4 = t1 + t3;
    const int z5 = (z3 + z4) * F1_175;
    t0 *= F0_298, t1 *= F2_053, t2 *= F3_072, t3 *= F1_501;
    z1 *= -F0_899, z2 *= -F2_562, z3 = z3 * -F1_961 + z5, z4 = z4 * -F0_390 + z5;
    t0 += z1 + z3, t1 += z2 + z4, t2 += z2 + z3, t3 += z1 + z4;
    d[0] = descale(t10 + t3, SHIFT), d[7 * S] = descale(t10 - t3, SHIFT);
    d[S] = descale(t11 + t2, SHIFT), d[6 * S] = descale(t11 - t2, SHIFT);
    d[2 * S] = descale(t12 + t1, SHIFT), d[5 * S] = descale(t12 - t1, SHIFT);
    d[3 * S] = descale(t13 + t0, SHIFT), d[4 * S] = descale(t13 - t0, SHIFT);
}

__global__ void __launch_bounds__(64)
jpegd_idct_kernel(const uint4 *__restrict__ coefs, const int *__restrict__ tables, uint8_t *__restrict__ planes, DGeom g, int total) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= total) return;
    const int n = i / g.nblk, b = i % g.nblk;
    const int mcu = b / g.bpm, j = b % g.bpm, ny = g.hs * g.vs;
    const int mr = mcu / g.mcus_per_row, mc = mcu % g.mcus_per_row;
    int comp = 0, by = mr, bx = mc;
    if (j < ny) by = mr * g.vs + j / g.hs, bx = mc * g.hs + j % g.hs;
    else comp = j - ny + 1;
    const int *q = tables + (long)n * TAB_WORDS + 64 * comp;
    int d[64];
    const uint4 *src = coefs + (long)i * 8;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const uint4 v = src[r];
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int coef = (int)(short)(w[c >> 1] >> (16 * (c & 1)));
            d[8 * r + c] = coef * (q[8 * r + c] & 0xffff);
        }
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) idct8<8, 11>(d + c);
#pragma unroll
    for (int r = 0; r < 8; ++r) idct8<1, 18>(d + 8 * r);
    uint8_t *dst = planes + (long)n * g.plane_bytes + g.po[comp] + ((long)by * 8) * g.pw[comp] + bx * 8;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        unsigned lo = 0, hi = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            lo |= (unsigned)min(max(d[8 * r + c] + 128, 0), 255) << (8 * c);
            hi |= (unsigned)min(max(d[8 * r + 4 + c] + 128, 0), 255) << (8 * c);
        }
        *reinterpret_cast<uint2 *>(dst + (long)r * g.pw[comp]) = make_uint2(lo, hi);       // planes are 8-byte tiled
    }
}

// ---- upsampling and colour ------------------------------------------------------------------------------------------------
// sample (y, x) of a chroma plane at full resolution
__device__ __forceinline__ int chroma_at(const uint8_t *pl, int pw, const DGeom &g, int y, int x) {
    if (g.hs == 1) return pl[(long)y * pw + x];
    if (g.dw <= 2) return pl[(long)(g.vs == 2 ? y >> 1 : y) * pw + (x >> 1)];
    const int i = x >> 1;
    if (g.vs == 2) {
        const int cy = y >> 1, fy = (y & 1) ? min(cy + 1, g.dh - 1) : max(cy - 1, 0);
        const uint8_t *near = pl + (long)cy * pw, *far = pl + (long)fy * pw;
        const int j = (x & 1) ? min(i + 1, g.dw - 1) : max(i - 1, 0);
        const int here = 3 * near[i] + far[i], there = 3 * near[j] + far[j];
        return (3 * here + there + ((x & 1) ? 7 : 8)) >> 4;
    }
    const uint8_t *row = pl + (long)y * pw;
    if (x == 0) return row[0];
    if (x == 2 * g.dw - 1) return row[g.dw - 1];
    return (x & 1) ? (3 * row[i] + row[i + 1] + 2) >> 2 : (3 * row[i] + row[i - 1] + 1) >> 2;
}

__device__ __forceinline__ uint8_t clamp_u8(int v) { return (uint8_t)min(max(v, 0), 255); }

__global__ void __launch_bounds__(PIX_THREADS)
jpegd_pixels_kernel(const uint8_t *__restrict__ planes, const int *__restrict__ seg_info, uint8_t *__restrict__ out,
                    int *__restrict__ status, DGeom g) {
    const int n = blockIdx.y;
    if (blockIdx.x == 0) {                              // the file's error bits: all of its segments'
        __shared__ int bits;
        if (threadIdx.x == 0) bits = 0;
        __syncthreads();
        int mine = 0;
        for (int s = threadIdx.x; s < g.n_seg; s += PIX_THREADS) mine |= seg_info[((long)n * g.n_seg + s) * 2];
        if (mine) atomicOr(&bits, mine);
        __syncthreads();
        if (threadIdx.x == 0) status[n] = bits;
    }
    const long i = (long)blockIdx.x * PIX_THREADS + threadIdx.x;
    if (i >= (long)g.H * g.W) return;
    const int y = (int)(i / g.W), x = (int)(i % g.W);
    const uint8_t *pl = planes + (long)n * g.plane_bytes;
    uint8_t *o = out + ((long)n * g.H * g.W + i) * g.C;
    const int lum = pl[g.po[0] + (long)y * g.pw[0] + x];
    if (g.ncomp == 1) {
        for (int c = 0; c < g.C; ++c) o[c] = (uint8_t)lum;
        return;
    }
    // jdcolor, 16 fraction bits, FIX(x) = int(x * 65536 + 0.5)
    const int cb = chroma_at(pl + g.po[1], g.pw[1], g, y, x) - 128, cr = chroma_at(pl + g.po[2], g.pw[2], g, y, x) - 128;
    o[0] = clamp_u8(lum + ((91881 * cr + 32768) >> 16));
    o[1] = clamp_u8(lum + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
    o[2] = clamp_u8(lum + ((116130 * cb + 32768) >> 16));
}

// ---- host ---------------------------------------------------------------------------------------------------------------
// IR2RGB_OK and the geometry, or IR2RGB_EINVAL
int geometry(int N, int C, int H, int W, int mode, int n_segments, DGeom *g) {
    if (n_segments < 1 || n_segments > 65535 || jpeg_grid(N, C, H, W, mode, g) != IR2RGB_OK) return IR2RGB_EINVAL;
    if ((long)N * n_segments > 0x7fffffffL / 8) return IR2RGB_EINVAL;
    g->n_seg = n_segments, g->ncomp = mode == MODE_L ? 1 : 3, g->n_mcus = g->mcus_per_row * g->mcu_rows;
    g->dw = (W + g->hs - 1) / g->hs, g->dh = (H + g->vs - 1) / g->vs;
    long off = 0;
    for (int c = 0; c < 3; ++c) {
        g->pw[c] = g->mcus_per_row * 8 * (c == 0 ? g->hs : 1), g->ph[c] = g->mcu_rows * 8 * (c == 0 ? g->vs : 1);
        g->po[c] = off;
        if (c < g->ncomp) off += (long)g->pw[c] * g->ph[c];
    }
    g->plane_bytes = align16(off);
    return IR2RGB_OK;
}

struct Workspace {
    long coefs, planes, info, bytes;        // byte offsets of the three regions, and the size
};
Workspace workspace_of(const DGeom &g, int N) {
    Workspace w;
    w.coefs = 0;
    w.planes = (long)N * g.nblk * 128;
    w.info = w.planes + (long)N * g.plane_bytes;
    w.bytes = w.info + (long)N * g.n_seg * 8;
    return w;
}

}  // namespace

extern "C" long ir2rgb_jpeg_decode_workspace_bytes(int N, int H, int W, int mode, int n_segments) {
    DGeom g;
    const int rc = geometry(N, mode == MODE_L ? 1 : 3, H, W, mode, n_segments, &g);
    if (rc != IR2RGB_OK) return rc;
    return workspace_of(g, N).bytes;
}

extern "C" int ir2rgb_jpeg_decode_u8(const uint8_t *files, const int *file_offsets, const int *segments, const int *tables,
                                     uint8_t *out, int *status, void *workspace, long workspace_bytes, int N, int C_out, int H,
                                     int W, int mode, int n_segments, int sub_bytes, void *stream) {
    DGeom g;
    const int rc = geometry(N, C_out, H, W, mode, n_segments, &g);
    if (rc != IR2RGB_OK) return rc;
    if (!files || !file_offsets || !segments || !tables || !out || !status || !workspace || sub_bytes < 1) return IR2RGB_EINVAL;
    const Workspace ws = workspace_of(g, N);
    if (workspace_bytes < ws.bytes) return IR2RGB_EINVAL;
    if (misaligned(workspace, 16) || misaligned(file_offsets, 4) || misaligned(segments, 4) || misaligned(tables, 4) ||
        misaligned(status, 4))
        return IR2RGB_EALIGN;
    hipStream_t s = as_stream(stream);
    uint8_t *base = static_cast<uint8_t *>(workspace);
    int16_t *coefs = reinterpret_cast<int16_t *>(base + ws.coefs);
    uint8_t *planes = base + ws.planes;
    int *info = reinterpret_cast<int *>(base + ws.info);
    jpegd_entropy_kernel<<<dim3(n_segments, N), ENT_THREADS, 0, s>>>(files, file_offsets, segments, tables, coefs, info, g, sub_bytes);
    const int total = N * g.nblk;
    jpegd_idct_kernel<<<cdiv(total, 64), 64, 0, s>>>(reinterpret_cast<const uint4 *>(coefs), tables, planes, g, total);
    const dim3 grid(cdiv((long)H * W, PIX_THREADS), N);
    jpegd_pixels_kernel<<<grid, PIX_THREADS, 0, s>>>(planes, info, out, status, g);
    return ir2rgb_launch_status();
}
