// video_metrics.hip -- SSIM and L2 scores of translated frames against ground truth, on the device, in fp64.
//
// The reference scores a movie with scripts/ssim_metric.py: skimage.color.rgb2gray of both uint8 frames, scikit-image's
// windowed SSIM (7x7 uniform window, sample covariance, K1 = 0.01, K2 = 0.03) with
// dynamic_range = original_gray.max() - predicted_gray.min(), and np.linalg.norm(original_gray - predicted_gray) as its
// "mse".  ir2rgb_video_metrics_u8 computes those per frame from two uint8 [N][H][W][3] batches in three launches:
//
//   metrics_reduce_kernel   grid (rows, N): grid-stride over the pixels of frame n; workgroup b writes the partial row
//                           [max gray(orig), min gray(pred), sum (gray(orig) - gray(pred))^2] at part1[n][b]
//   metrics_ssim_kernel     grid (tiles, N): one workgroup per TR x TC tile of the (H-6) x (W-6) window grid.  It recomputes
//                           the haloed (TR+6) x (TC+6) gray tile of both images from the bytes into LDS (this second read
//                           comes out of L2 / Infinity Cache), reduces frame n's rows of part1 to R, forms the five window
//                           sums separably (7 along the row into LDS, then 7 down the column), evaluates S per window and
//                           writes the tile's sum of S to part2[n][tile]
//   metrics_finish_kernel   grid (N): sums part2[n][*], part1[n][*] and writes out[n] = {ssim, l2, R}
//
// Nothing is padded: scikit-image filters with reflected borders and then crops 3 pixels, so the values it averages are
// exactly the windows that lie inside the image.  There are no special cases either: R <= 0, flat images and 0/0 give
// what IEEE arithmetic gives in NumPy (an all-black pair scores NaN).
//
// Arithmetic: contraction is off for the whole file, and every expression is written in the operation order of
// ir2rgb_amd.metrics.ssim_reference (gray from the bytes, row sums left to right, column sums top to bottom, one division
// by 49, the variance and S formulas as scikit-image spells them).  Per window the kernel therefore performs the same
// IEEE operations as the torch restatement; the two differ only in the order of the long sums (sum of d^2, sum of S).
// Those sums have a fixed order (per thread in index order, then a binary tree over the workgroup, then the same over the
// partials): no atomics, results are bit-reproducible run to run.
//
// Loads: every global load of a thread is issued before the first use, from an address clamped into the frame, and masked
// afterwards (a duplicate pixel changes neither a max nor a min; sums select 0).  A tile workgroup has 4 x 6 byte loads and
// 2 partial loads per thread in flight, a reduce thread 4 x 6 dwords (rows of 4 pixels as 3 dwords when H*W is a multiple
// of 4 and the bases are dword aligned) or 4 x 6 bytes per trip.  46 to 74 VGPRs, no scratch.
#include "common.h"
#include "reduce.h"     // block_reduce, partial_rows, frame_sizes_ok
#include "u8.h"         // get_byte

#pragma clang fp contract(off)

namespace {

constexpr int BLOCK = 256;
constexpr int TR = 16, TC = 32;             // windows (output pixels) per tile
constexpr int HR = TR + 6, HC = TC + 6;     // gray pixels a tile needs
constexpr int NP = (HR * HC + BLOCK - 1) / BLOCK;   // haloed pixels per thread
constexpr int P1_UNROLL = 4;                // groups per thread and trip of the reduce pass
constexpr int P1_PIXELS = BLOCK * 16;       // pixels per partial row before a workgroup takes a second trip
constexpr int P1_MAX_ROWS = BLOCK;          // one partial row per thread of the passes that read them
constexpr int MIN_SIDE = 7;                 // one window

__device__ __forceinline__ double gray(unsigned r, unsigned g, unsigned b) {
    // skimage.color.rgb2gray of a uint8 image: img_as_float (v / 255), then the dot product with the weights
    return ((double)r / 255.0) * 0.2125 + ((double)g / 255.0) * 0.7154 + ((double)b / 255.0) * 0.0721;
}

// PPG pixels per group: 4 (their 12 bytes as 3 dwords; hw % 4 == 0, dword-aligned bases) or 1 (3 bytes)
template <int PPG>
__global__ void __launch_bounds__(BLOCK)
metrics_reduce_kernel(const uint8_t *__restrict__ orig, const uint8_t *__restrict__ pred, double *__restrict__ part1, long hw) {
    __shared__ double red[BLOCK];
    const int n = blockIdx.y, rows = gridDim.x, tid = threadIdx.x;
    const uint8_t *fo = orig + (long)n * hw * 3, *fp = pred + (long)n * hw * 3;
    const long groups = hw / PPG;
    double mx = -INFINITY, mn = INFINITY, ss = 0.0;
    for (long base = (long)blockIdx.x * (BLOCK * P1_UNROLL); base < groups; base += (long)rows * (BLOCK * P1_UNROLL)) {
        unsigned bo[P1_UNROLL][3], bp[P1_UNROLL][3];
#pragma unroll
        for (int u = 0; u < P1_UNROLL; ++u) {
            const long g = base + u * BLOCK + tid;
            const long gc = g < groups ? g : groups - 1;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (PPG == 4) {
                    bo[u][k] = reinterpret_cast<const unsigned *>(fo)[gc * 3 + k];
                    bp[u][k] = reinterpret_cast<const unsigned *>(fp)[gc * 3 + k];
                } else {
                    bo[u][k] = fo[gc * 3 + k];
                    bp[u][k] = fp[gc * 3 + k];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < P1_UNROLL; ++u) {
            const bool valid = base + u * BLOCK + tid < groups;
#pragma unroll
            for (int p = 0; p < PPG; ++p) {
                unsigned co[3], cp[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    co[c] = PPG == 4 ? get_byte(bo[u], p * 3 + c) : bo[u][c];
                    cp[c] = PPG == 4 ? get_byte(bp[u], p * 3 + c) : bp[u][c];
                }
                const double go = gray(co[0], co[1], co[2]), gp = gray(cp[0], cp[1], cp[2]);
                const double d = go - gp;
                mx = fmax(mx, go);              // a clamped (repeated) pixel changes neither extreme
                mn = fmin(mn, gp);
                ss += valid ? d * d : 0.0;
            }
        }
    }
    mx = block_reduce<REDUCE_MAX, BLOCK>(mx, red);
    mn = block_reduce<REDUCE_MIN, BLOCK>(mn, red);
    ss = block_reduce<REDUCE_SUM, BLOCK>(ss, red);
    if (tid == 0) {
        double *row = part1 + ((long)n * rows + blockIdx.x) * 3;
        row[0] = mx, row[1] = mn, row[2] = ss;
    }
}

__global__ void __launch_bounds__(BLOCK)
metrics_ssim_kernel(const uint8_t *__restrict__ orig, const uint8_t *__restrict__ pred, const double *__restrict__ range,
                    const double *__restrict__ part1, double *__restrict__ part2, int H, int W, int rows, int tiles_x) {
    __shared__ double gx[HR * HC], gy[HR * HC], hs[5][HR * TC], red[BLOCK];
    const int n = blockIdx.y, tile = blockIdx.x, tiles = gridDim.x, tid = threadIdx.x;
    const int y0 = (tile / tiles_x) * TR, x0 = (tile % tiles_x) * TC;
    const long hw = (long)H * W;
    const uint8_t *fo = orig + (long)n * hw * 3, *fp = pred + (long)n * hw * 3;

    unsigned bo[NP][3], bp[NP][3];
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const int p = min(tid + k * BLOCK, HR * HC - 1);
        const int y = min(y0 + p / HC, H - 1), x = min(x0 + p % HC, W - 1);
        const long off = ((long)y * W + x) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) bo[k][c] = fo[off + c], bp[k][c] = fp[off + c];
    }
    const double *row = part1 + ((long)n * rows + min(tid, rows - 1)) * 3;
    const double pmx = row[0], pmn = row[1];
    const double given = range ? range[n] : 0.0;        // (uniform over the launch)
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const int p = tid + k * BLOCK;
        if (p < HR * HC) {
            gx[p] = gray(bo[k][0], bo[k][1], bo[k][2]);
            gy[p] = gray(bp[k][0], bp[k][1], bp[k][2]);
        }
    }
    const double mx = block_reduce<REDUCE_MAX, BLOCK>(tid < rows ? pmx : -INFINITY, red);     // (its barriers also publish gx / gy)
    const double mn = block_reduce<REDUCE_MIN, BLOCK>(tid < rows ? pmn : INFINITY, red);
    const double R = range ? given : mx - mn;
    const double C1 = (0.01 * R) * (0.01 * R), C2 = (0.03 * R) * (0.03 * R);

    // 7 along the row: x, y, x*x, y*y, x*y
    for (int i = tid; i < HR * TC; i += BLOCK) {
        const double *px = gx + (i / TC) * HC + i % TC, *py = gy + (i / TC) * HC + i % TC;
        double sx = px[0], sy = py[0], sxx = px[0] * px[0], syy = py[0] * py[0], sxy = px[0] * py[0];
#pragma unroll
        for (int k = 1; k < 7; ++k) {
            sx += px[k], sy += py[k], sxx += px[k] * px[k], syy += py[k] * py[k], sxy += px[k] * py[k];
        }
        hs[0][i] = sx, hs[1][i] = sy, hs[2][i] = sxx, hs[3][i] = syy, hs[4][i] = sxy;
    }
    __syncthreads();

    // 7 down the column, the means, S
    double acc = 0.0;
    for (int o = tid; o < TR * TC; o += BLOCK) {
        const int r = o / TC, c = o % TC;
        double m[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            double s = hs[q][r * TC + c];
#pragma unroll
            for (int k = 1; k < 7; ++k) s += hs[q][(r + k) * TC + c];
            m[q] = s / 49.0;
        }
        const double ux = m[0], uy = m[1], uxx = m[2], uyy = m[3], uxy = m[4];
        const double cov_norm = 49.0 / 48.0;
        const double vx = cov_norm * (uxx - ux * ux), vy = cov_norm * (uyy - uy * uy), vxy = cov_norm * (uxy - ux * uy);
        const double A1 = 2.0 * ux * uy + C1, A2 = 2.0 * vxy + C2, B1 = ux * ux + uy * uy + C1, B2 = vx + vy + C2;
        const double S = (A1 * A2) / (B1 * B2);
        acc += (y0 + r < H - 6 && x0 + c < W - 6) ? S : 0.0;
    }
    acc = block_reduce<REDUCE_SUM, BLOCK>(acc, red);
    if (tid == 0) part2[(long)n * tiles + tile] = acc;
}

__global__ void __launch_bounds__(BLOCK)
metrics_finish_kernel(const double *__restrict__ range, const double *__restrict__ part1, const double *__restrict__ part2,
                      double *__restrict__ out, int rows, int tiles, long windows) {
    __shared__ double red[BLOCK];
    const int n = blockIdx.x, tid = threadIdx.x;
    const double *row = part1 + ((long)n * rows + min(tid, rows - 1)) * 3;
    const double pmx = row[0], pmn = row[1], pss = row[2];
    const double given = range ? range[n] : 0.0;
    const double *tp = part2 + (long)n * tiles;
    double acc = 0.0;
    for (int base = 0; base < tiles; base += BLOCK * 8) {
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = tp[min(base + u * BLOCK + tid, tiles - 1)];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += base + u * BLOCK + tid < tiles ? v[u] : 0.0;
    }
    acc = block_reduce<REDUCE_SUM, BLOCK>(acc, red);
    const double mx = block_reduce<REDUCE_MAX, BLOCK>(tid < rows ? pmx : -INFINITY, red);
    const double mn = block_reduce<REDUCE_MIN, BLOCK>(tid < rows ? pmn : INFINITY, red);
    const double ss = block_reduce<REDUCE_SUM, BLOCK>(tid < rows ? pss : 0.0, red);
    if (tid == 0) {
        out[(long)n * 3 + 0] = acc / (double)windows;
        out[(long)n * 3 + 1] = sqrt(ss);
        out[(long)n * 3 + 2] = range ? given : mx - mn;
    }
}

inline int tiles_x(int W) { return (W - 6 + TC - 1) / TC; }
inline int tiles_y(int H) { return (H - 6 + TR - 1) / TR; }

}  // namespace

extern "C" long ir2rgb_video_metrics_workspace_bytes(int N, int H, int W) {
    if (!frame_sizes_ok(N, H, W, MIN_SIDE)) return IR2RGB_EINVAL;
    return (long)sizeof(double) * N * (3L * partial_rows((long)H * W, P1_PIXELS, P1_MAX_ROWS) + (long)tiles_x(W) * tiles_y(H));
}

extern "C" int ir2rgb_video_metrics_tile(int which) {
    return which == 0 ? TR : (which == 1 ? TC : IR2RGB_EINVAL);
}

extern "C" int ir2rgb_video_metrics_u8(const uint8_t *orig, const uint8_t *pred, const double *range, double *out,
                                       void *workspace, long workspace_bytes, int N, int H, int W, void *stream) {
    if (!orig || !pred || !out || !workspace || !frame_sizes_ok(N, H, W, MIN_SIDE)) return IR2RGB_EINVAL;
    if (workspace_bytes < ir2rgb_video_metrics_workspace_bytes(N, H, W)) return IR2RGB_EINVAL;
    if (misaligned(out, 8) || misaligned(range, 8) || misaligned(workspace, 8)) return IR2RGB_EALIGN;
    const long hw = (long)H * W;
    const int rows = partial_rows(hw, P1_PIXELS, P1_MAX_ROWS), tx = tiles_x(W), tiles = tx * tiles_y(H);
    double *part1 = static_cast<double *>(workspace), *part2 = part1 + (long)N * rows * 3;
    hipStream_t s = as_stream(stream);
    with_bool(hw % 4 == 0 && !misaligned(orig, 4) && !misaligned(pred, 4), [&](auto wide) {
        metrics_reduce_kernel<wide.value ? 4 : 1><<<dim3(rows, N), BLOCK, 0, s>>>(orig, pred, part1, hw);
    });
    metrics_ssim_kernel<<<dim3(tiles, N), BLOCK, 0, s>>>(orig, pred, range, part1, part2, H, W, rows, tx);
    metrics_finish_kernel<<<N, BLOCK, 0, s>>>(range, part1, part2, out, rows, tiles, (long)(H - 6) * (W - 6));
    return ir2rgb_launch_status();
}
