// jpeg_common.h -- the vocabulary the two halves of the baseline JPEG codec share, each fact stated once.
// Users: jpeg.hip (frames -> files) and jpeg_decode.hip (files -> frames).  The Python side of the same list is
// ir2rgb_amd/jpeg_common.py: ZIGZAG is ZZ, the keys of F are the multipliers below, Geometry is jpeg_grid.
#pragma once
#include "common.h"

constexpr int MODE_444 = IR2RGB_JPEG_444, MODE_420 = IR2RGB_JPEG_420, MODE_L = IR2RGB_JPEG_L, MODE_422 = IR2RGB_JPEG_422;

// natural index of zigzag position k
static __device__ constexpr unsigned char ZZ[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,
                                                    12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                                    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
                                                    58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// jfdctint / jidctint: FIX(x) with CONST_BITS 13, named after x as the keys of Python's F are
constexpr int F0_298 = 2446, F0_390 = 3196, F0_541 = 4433, F0_765 = 6270, F0_899 = 7373, F1_175 = 9633, F1_501 = 12299,
              F1_847 = 15137, F1_961 = 16069, F2_053 = 16819, F2_562 = 20995, F3_072 = 25172;

static __device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// inclusive sum over the values of a workgroup of THREADS in a fixed order (sh: THREADS ints of LDS); *total: the sum of all
template <int THREADS> __device__ __forceinline__ int scan_inclusive(int v, int *sh, int *total) {
    const int t = threadIdx.x;
    __syncthreads();
    sh[t] = v;
    __syncthreads();
    for (int d = 1; d < THREADS; d <<= 1) {
        const int x = t >= d ? sh[t - d] : 0;
        __syncthreads();
        sh[t] += x;
        __syncthreads();
    }
    *total = sh[THREADS - 1];
    return sh[t];
}

// ---- host ---------------------------------------------------------------------------------------------------------------
static inline long align16(long v) { return (v + 15) & ~15L; }

// The MCU grid of a frame: what the geometry of either direction starts with (and its kernels read under these names).
struct JpegGrid {
    int H, W, C, mode;
    int hs, vs;                 // luminance sampling factors: an MCU is 8 hs x 8 vs pixels
    int bpm;                    // blocks per MCU
    int mcus_per_row, mcu_rows;
    int nblk;                   // blocks per frame
};

// IR2RGB_OK and the grid of N frames [H][W][C] of one mode, or IR2RGB_EINVAL.  N rides in gridDim.y, a side is a 16-bit
// field of the frame header, and a coefficient of the N frames' blocks is addressed in int.
static inline int jpeg_grid(int N, int C, int H, int W, int mode, JpegGrid *g) {
    if (N < 1 || N > 65535 || H < 1 || W < 1 || H > 65535 || W > 65535) return IR2RGB_EINVAL;
    if (mode < MODE_444 || mode > MODE_422 || (C != 1 && C != 3) || (mode != MODE_L && C != 3)) return IR2RGB_EINVAL;
    g->H = H, g->W = W, g->C = C, g->mode = mode;
    g->hs = (mode == MODE_420 || mode == MODE_422) ? 2 : 1;
    g->vs = mode == MODE_420 ? 2 : 1;
    g->bpm = mode == MODE_L ? 1 : g->hs * g->vs + 2;
    g->mcus_per_row = (W + 8 * g->hs - 1) / (8 * g->hs), g->mcu_rows = (H + 8 * g->vs - 1) / (8 * g->vs);
    const long nblk = (long)g->mcu_rows * g->mcus_per_row * g->bpm;
    if (nblk * N > 0x7fffffffL / 64) return IR2RGB_EINVAL;
    g->nblk = (int)nblk;
    return IR2RGB_OK;
}
