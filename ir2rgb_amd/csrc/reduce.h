// reduce.h -- what the per-frame reductions share: the fixed-order fp64 workgroup tree that makes the scores of
// video_metrics.hip and warp_error.hip bit-reproducible, the partial-row rule (also visuals.hip) and the frame-size check.
#pragma once
#include <hip/hip_runtime.h>

enum { REDUCE_SUM = 0, REDUCE_MAX = 1, REDUCE_MIN = 2 };

// fixed-order binary tree over a workgroup of BLOCK threads (sh: BLOCK doubles of LDS); every thread returns the total
template <int OP, int BLOCK>
__device__ __forceinline__ double block_reduce(double v, double *sh) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int s = BLOCK / 2; s > 0; s >>= 1) {
        if (t < s) {
            const double a = sh[t], b = sh[t + s];
            sh[t] = OP == REDUCE_SUM ? a + b : (OP == REDUCE_MAX ? fmax(a, b) : fmin(a, b));
        }
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

// partial rows of a frame of hw pixels: one workgroup, and one row of partial results, per pixels_per_row pixels, at most
// max_rows (the pass that folds the rows gives each of its threads one)
static inline int partial_rows(long hw, int pixels_per_row, int max_rows) {
    const long r = (hw + pixels_per_row - 1) / pixels_per_row;
    return (int)(r > max_rows ? max_rows : r);
}

// N rides in gridDim.y; offsets inside a frame of three bytes per pixel stay below 2^31
static inline bool frame_sizes_ok(int N, int H, int W, int min_side) {
    return N >= 1 && N <= 65535 && H >= min_side && W >= min_side && (long)H * W * 3 <= 0x7fffffffL;
}
