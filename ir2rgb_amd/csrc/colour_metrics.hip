// colour_metrics.hip -- colour fidelity of a translated video: RGB PSNR and the CIELAB error of frames, on the device, in fp64.
//
// The other scores are blind to colour: video_metrics.hip works on rgb2gray, warp_error.hip measures flicker.
// ir2rgb_colour_metrics_u8 scores pred against orig, uint8 [N][H][W][3] both, per frame.  For every pixel of either frame,
// everything in fp64 (the constants are scikit-image's rgb2lab: D65, 2 degree observer):
//
//   r, g, b = lin[R], lin[G], lin[B]        lin: the caller's 256 doubles, the sRGB decoding of a byte (v/255 -> c/12.92 or
//                                           ((c + 0.055)/1.055)^2.4), formed once on the host: pow never runs here
//   tX = (0.412453 r + 0.357580 g + 0.180423 b) / 0.95047          products and sums left to right, then the division
//   tY = (0.212671 r + 0.715160 g + 0.072169 b) / 1.0
//   tZ = (0.019334 r + 0.119193 g + 0.950227 b) / 1.08883
//   f(t) = cbrt(t) if t > 0.008856 else 7.787 t + 16/116
//   L = 116 f(tY) - 16,  a = 500 (f(tX) - f(tY)),  b = 200 (f(tY) - f(tZ))
//
// and with dL, da, db the differences orig - pred of a pixel:
//
//   dE = sqrt(dL dL + da da + db db)   (CIE76)        dC = sqrt(da da + db db)   (the distance in the colour plane)
//   SSE = sum (orig - pred)^2 over pixels and channels, in byte units
//   out[n] = { mse = SSE / (3 H W),  psnr = 10 log10(65025 / mse),  sum dE / (H W),  sum |dL| / (H W),  sum dC / (H W) }
//
// Two launches:
//   colour_reduce_kernel   grid (rows, N): grid-stride over the pixels of frame n, 4 pixels per thread and trip; workgroup b
//                          writes the partial row [SSE, sum dE, sum |dL|, sum dC] at part[n][b]
//   colour_finish_kernel   grid (N): sums part[n][*] (at most 256 rows) and writes out[n]
//
// There are no special cases: both frames go through the same arithmetic, so identical frames give mse = 0,
// psnr = 10 log10(65025 / 0) = +inf and exact zeros in the three Lab columns.
//
// Arithmetic: contraction is off for the whole file and every expression is written in the operation order of
// ir2rgb_amd.metrics.colour_reference; the two differ in the library cube root and in the order of the three long Lab sums.
// SSE is a sum of integers that stays below 2^53: it is the same double in any order.  The sums have a fixed order (per
// thread in index order, a binary tree over the workgroup, the same over the partial rows): no atomics, results are
// bit-reproducible, frames never mix.  The only library functions are cbrt (six per pixel), sqrt and one log10 per frame.
//
// Loads: every thread first copies one entry of lin into a 2 KB LDS table.  Per trip the bytes of both frames are issued
// first, then used.  Tail lanes load from a clamped group and select 0 afterwards.  With W % 4 == 0 and 4-byte aligned bases
// a thread's 4 pixels are one group, its 12 bytes per frame three dwords; otherwise the same code runs on 4 groups of one pixel.
#include "common.h"
#include "reduce.h"     // block_reduce, partial_rows, frame_sizes_ok
#include "u8.h"         // get_byte

#pragma clang fp contract(off)

namespace {

constexpr int BLOCK = 256;                      // also the entries of lin: one per thread
constexpr int PPT = 4;                          // pixels per thread and trip
constexpr int ROW_PIXELS = BLOCK * PPT;         // pixels per partial row: one trip each until MAX_ROWS workgroups per frame
constexpr int MAX_ROWS = BLOCK;                 // one partial row per thread of the finish pass
constexpr int COLS = 4;                         // doubles per partial row
constexpr int MIN_SIDE = 1;

struct Lab {
    double L, a, b;
};

__device__ __forceinline__ double lab_f(double t) { return t > 0.008856 ? cbrt(t) : 7.787 * t + 16.0 / 116.0; }

// one pixel from its three bytes; tab: lin in LDS
__device__ __forceinline__ Lab to_lab(const double *tab, unsigned R, unsigned G, unsigned B) {
    const double r = tab[R], g = tab[G], b = tab[B];
    const double tx = (0.412453 * r + 0.357580 * g + 0.180423 * b) / 0.95047;
    const double ty = (0.212671 * r + 0.715160 * g + 0.072169 * b) / 1.0;
    const double tz = (0.019334 * r + 0.119193 * g + 0.950227 * b) / 1.08883;
    const double fx = lab_f(tx), fy = lab_f(ty), fz = lab_f(tz);
    Lab v;
    v.L = 116.0 * fy - 16.0;
    v.a = 500.0 * (fx - fy);
    v.b = 200.0 * (fy - fz);
    return v;
}

// PPG pixels per group: 4 (12 bytes of either frame as 3 dwords; W % 4 == 0, aligned bases) or 1
template <int PPG>
__global__ void __launch_bounds__(BLOCK)
colour_reduce_kernel(const uint8_t *__restrict__ orig, const uint8_t *__restrict__ pred, const double *__restrict__ lin,
                     double *__restrict__ part, int H, int W) {
    __shared__ double red[BLOCK];
    __shared__ double tab[BLOCK];
    constexpr int U = PPT / PPG;                // groups per thread and trip
    const int n = blockIdx.y, rows = gridDim.x, tid = threadIdx.x;
    tab[tid] = lin[tid];
    __syncthreads();
    const int hw = H * W;                       // 3 * hw < 2^31: offsets inside a frame are ints
    const uint8_t *fo = orig + (long)n * hw * 3, *fp = pred + (long)n * hw * 3;
    const int groups = hw / PPG;
    double sse = 0.0, se = 0.0, sl = 0.0, sc = 0.0;
    for (int base = blockIdx.x * (BLOCK * U); base < groups; base += rows * (BLOCK * U)) {
        unsigned ob[U][3], pb[U][3];
        bool valid[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int g = base + u * BLOCK + tid;
            valid[u] = g < groups;
            const int gc = valid[u] ? g : groups - 1;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (PPG == 4) {
                    ob[u][k] = reinterpret_cast<const unsigned *>(fo)[gc * 3 + k];
                    pb[u][k] = reinterpret_cast<const unsigned *>(fp)[gc * 3 + k];
                } else {
                    ob[u][k] = fo[gc * 3 + k];
                    pb[u][k] = fp[gc * 3 + k];
                }
            }
        }
#pragma unroll
        for (int q = 0; q < PPT; ++q) {
            const int u = q / PPG, p = q % PPG;
            unsigned o[3], v[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                o[c] = PPG == 4 ? get_byte(ob[u], p * 3 + c) : ob[u][c];
                v[c] = PPG == 4 ? get_byte(pb[u], p * 3 + c) : pb[u][c];
            }
            double sq = 0.0;                    // integers <= 3 * 255^2: exact
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double d = (double)o[c] - (double)v[c];
                sq += d * d;
            }
            const Lab lo = to_lab(tab, o[0], o[1], o[2]), lp = to_lab(tab, v[0], v[1], v[2]);
            const double dL = lo.L - lp.L, da = lo.a - lp.a, db = lo.b - lp.b;
            const double de = sqrt(dL * dL + da * da + db * db), dc = sqrt(da * da + db * db);
            sse += valid[u] ? sq : 0.0;
            se += valid[u] ? de : 0.0;
            sl += valid[u] ? fabs(dL) : 0.0;
            sc += valid[u] ? dc : 0.0;
        }
    }
    sse = block_reduce<REDUCE_SUM, BLOCK>(sse, red);
    se = block_reduce<REDUCE_SUM, BLOCK>(se, red);
    sl = block_reduce<REDUCE_SUM, BLOCK>(sl, red);
    sc = block_reduce<REDUCE_SUM, BLOCK>(sc, red);
    if (tid == 0) {
        double *row = part + ((long)n * rows + blockIdx.x) * COLS;
        row[0] = sse, row[1] = se, row[2] = sl, row[3] = sc;
    }
}

__global__ void __launch_bounds__(BLOCK)
colour_finish_kernel(const double *__restrict__ part, double *__restrict__ out, int rows, int H, int W) {
    __shared__ double red[BLOCK];
    const int n = blockIdx.x, tid = threadIdx.x;
    const double *row = part + ((long)n * rows + min(tid, rows - 1)) * COLS;
    const double p0 = row[0], p1 = row[1], p2 = row[2], p3 = row[3];
    const double sse = block_reduce<REDUCE_SUM, BLOCK>(tid < rows ? p0 : 0.0, red);
    const double se = block_reduce<REDUCE_SUM, BLOCK>(tid < rows ? p1 : 0.0, red);
    const double sl = block_reduce<REDUCE_SUM, BLOCK>(tid < rows ? p2 : 0.0, red);
    const double sc = block_reduce<REDUCE_SUM, BLOCK>(tid < rows ? p3 : 0.0, red);
    if (tid == 0) {
        const double hw = (double)H * (double)W;
        const double mse = sse / (3.0 * hw);
        double *o = out + (long)n * 5;
        o[0] = mse;
        o[1] = 10.0 * log10(65025.0 / mse);
        o[2] = se / hw;
        o[3] = sl / hw;
        o[4] = sc / hw;
    }
}

}  // namespace

extern "C" long ir2rgb_colour_metrics_workspace_bytes(int N, int H, int W) {
    if (!frame_sizes_ok(N, H, W, MIN_SIDE)) return IR2RGB_EINVAL;
    return (long)sizeof(double) * N * COLS * partial_rows((long)H * W, ROW_PIXELS, MAX_ROWS);
}

extern "C" int ir2rgb_colour_metrics_u8(const uint8_t *orig, const uint8_t *pred, const double *lin, double *out,
                                        void *workspace, long workspace_bytes, int N, int H, int W, void *stream) {
    if (!orig || !pred || !lin || !out || !workspace || !frame_sizes_ok(N, H, W, MIN_SIDE)) return IR2RGB_EINVAL;
    if (workspace_bytes < ir2rgb_colour_metrics_workspace_bytes(N, H, W)) return IR2RGB_EINVAL;
    if (misaligned(out, 8) || misaligned(lin, 8) || misaligned(workspace, 8)) return IR2RGB_EALIGN;
    const int rows = partial_rows((long)H * W, ROW_PIXELS, MAX_ROWS);
    double *part = static_cast<double *>(workspace);
    hipStream_t s = as_stream(stream);
    const bool wide = W % 4 == 0 && !misaligned(orig, 4) && !misaligned(pred, 4);
    with_bool(wide, [&](auto wd) {
        colour_reduce_kernel<wd.value ? 4 : 1><<<dim3(rows, N), BLOCK, 0, s>>>(orig, pred, lin, part, H, W);
    });
    colour_finish_kernel<<<N, BLOCK, 0, s>>>(part, out, rows, H, W);
    return ir2rgb_launch_status();
}
