// warp_error.hip -- temporal consistency of a translated video: the warp error of consecutive frames, on the device, in fp64.
//
// The trainer penalises flicker with G_Warp = masked_l1(fake_B, resample(fake_B_prev, flow_ref), conf_ref)
// (reference models/discriminator.py:137-138, MaskedL1Loss, Model.resample in base_model.py:129-136).
// ir2rgb_warp_error_u8 computes that quantity, and the masked mean squared error beside it, per pair of uint8 frames:
// prev, cur [N][H][W][3], flow fp32 [N][2][H][W] (x then y, pixels, from cur to prev), weight fp32 [N][1][H][W] or NULL (= 1).
// For pixel (y, x), everything in fp64:
//
//   gx = (-1 + x * (2 / (W - 1))) + fx / ((W - 1) / 2)        get_grid's lattice (an align_corners=True one) plus the flow
//   ix = ((gx + 1) * W - 1) * 0.5, clamped to [0, W - 1]      grid_sample(align_corners=False, padding_mode="border"): the
//                                                             reference's mismatch, reproduced as warp_blend (heads.hip) does
//   x0 = floor(ix), x1 = min(x0 + 1, W - 1), ax = ix - x0     likewise y0, y1, ay from fy and H
//   w_c = (1-ay)(1-ax) prev[y0][x0][c] + (1-ay) ax prev[y0][x1][c] + ay (1-ax) prev[y1][x0][c] + ay ax prev[y1][x1][c]
//   d_c = cur[y][x][c] - w_c                                  byte units
//   S1 = sum m |d_c|,  S2 = sum m d_c^2  (pixels and channels),  SC = sum m  (pixels)
//   out[n] = { S1 / (127.5 * 3 * H * W),  S2 / (255^2 * 3 * SC),  SC / (H * W) }     warp_l1, warp_mse, coverage
//
// Two launches:
//   warp_reduce_kernel   grid (rows, N): grid-stride over the pixels of pair n, 4 pixels per thread and trip; workgroup b
//                        writes the partial row [S1, S2, SC] at part[n][b]
//   warp_finish_kernel   grid (N): sums part[n][*] (at most 256 rows) and writes out[n]
//
// There are no special cases: SC = 0 gives 0/0 = NaN, a NaN flow vector or weight stays in the sums of its own pair, an
// infinite flow vector lands on the border as any large one does.  No address leaves the frame whatever the flow holds: the
// coordinate is clamped in fp64 with comparisons that keep a NaN (so the weights ax, ay carry it), the index is taken from
// it with NaN -> 0 and clamped again as an integer.
//
// Arithmetic: contraction is off for the whole file and every expression is written in the operation order of
// ir2rgb_amd.metrics.warp_error_reference; the two differ only in the order of the three long sums.  Those have a fixed
// order (per thread in index order, a binary tree over the workgroup, the same over the partial rows): no atomics, results
// are bit-reproducible, pairs never mix.
//
// Loads: flow x and y, the weight and the bytes of cur are issued first, the coordinates formed, then the 4 x 3 bytes of
// prev of every pixel of the trip from their clamped addresses, and only then is the first of them used.  Tail lanes load
// from a clamped group and select 0 afterwards.  With W % 4 == 0 and aligned bases a thread's 4 pixels are one group: flow
// and weight as 16-byte loads, the 12 bytes of cur as three dwords (a group never crosses a row); otherwise the same code
// runs on 4 groups of one pixel.
#include "common.h"
#include "reduce.h"     // block_reduce, partial_rows, frame_sizes_ok
#include "u8.h"         // get_byte, unpack4

#pragma clang fp contract(off)

namespace {

constexpr int BLOCK = 256;
constexpr int PPT = 4;                          // pixels per thread and trip
constexpr int ROW_PIXELS = BLOCK * PPT;         // pixels per partial row: one trip each until MAX_ROWS workgroups per pair
constexpr int MAX_ROWS = BLOCK;                 // one partial row per thread of the finish pass
constexpr int MIN_SIDE = 2;                     // the lattice divides by W - 1 and H - 1

struct Coord {
    double a;       // weight of the second neighbour (NaN when the coordinate is)
    int i0, i1;     // both in [0, n - 1]
};

// one axis: lattice position i of n, flow component f in pixels
__device__ __forceinline__ Coord coord(int i, float f, int n) {
    const double g = (-1.0 + (double)i * (2.0 / (double)(n - 1))) + (double)f / ((double)(n - 1) / 2.0);
    double p = ((g + 1.0) * (double)n - 1.0) * 0.5;
    p = p < 0.0 ? 0.0 : (p > (double)(n - 1) ? (double)(n - 1) : p);       // comparisons: a NaN stays
    const double fl = floor(p);
    Coord c;
    c.a = p - fl;
    const int i0 = fl == fl ? (int)fl : 0;                                  // NaN -> 0
    c.i0 = min(max(i0, 0), n - 1);
    c.i1 = min(c.i0 + 1, n - 1);
    return c;
}

// PPG pixels per group: 4 (16-byte loads of flow and weight, cur as 3 dwords; W % 4 == 0, aligned bases) or 1
template <int PPG, bool HAS_W>
__global__ void __launch_bounds__(BLOCK)
warp_reduce_kernel(const uint8_t *__restrict__ prev, const uint8_t *__restrict__ cur, const float *__restrict__ flow,
                   const float *__restrict__ weight, double *__restrict__ part, int H, int W) {
    __shared__ double red[BLOCK];
    constexpr int U = PPT / PPG;                // groups per thread and trip
    const int n = blockIdx.y, rows = gridDim.x, tid = threadIdx.x;
    const int hw = H * W;                       // 3 * hw < 2^31: offsets inside a pair are ints
    const uint8_t *fp = prev + (long)n * hw * 3, *fc = cur + (long)n * hw * 3;
    const float *fx = flow + (long)n * hw * 2, *fy = fx + hw;
    const float *fw = HAS_W ? weight + (long)n * hw : nullptr;
    const int groups = hw / PPG;
    double s1 = 0.0, s2 = 0.0, sc = 0.0;
    for (int base = blockIdx.x * (BLOCK * U); base < groups; base += rows * (BLOCK * U)) {
        float vx[PPT], vy[PPT], vw[PPT];
        unsigned cb[U][3], pb[PPT][4][3];
        Coord cx[PPT], cy[PPT];
        bool valid[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int g = base + u * BLOCK + tid;
            valid[u] = g < groups;
            const int gc = valid[u] ? g : groups - 1;
            if (PPG == 4) {
                const float4 a = reinterpret_cast<const float4 *>(fx)[gc], b = reinterpret_cast<const float4 *>(fy)[gc];
                unpack4(a, vx), unpack4(b, vy);
                if (HAS_W) unpack4(reinterpret_cast<const float4 *>(fw)[gc], vw);
#pragma unroll
                for (int k = 0; k < 3; ++k) cb[u][k] = reinterpret_cast<const unsigned *>(fc)[gc * 3 + k];
            } else {
                vx[u] = fx[gc], vy[u] = fy[gc];
                if (HAS_W) vw[u] = fw[gc];
#pragma unroll
                for (int k = 0; k < 3; ++k) cb[u][k] = fc[gc * 3 + k];
            }
        }
#pragma unroll
        for (int q = 0; q < PPT; ++q) {
            const int g = base + (q / PPG) * BLOCK + tid;
            const int pix = (g < groups ? g : groups - 1) * PPG + q % PPG;
            const int y = pix / W, x = pix - y * W;
            cx[q] = coord(x, vx[q], W);
            cy[q] = coord(y, vy[q], H);
        }
#pragma unroll
        for (int q = 0; q < PPT; ++q) {
            const int o00 = (cy[q].i0 * W + cx[q].i0) * 3, o01 = (cy[q].i0 * W + cx[q].i1) * 3;
            const int o10 = (cy[q].i1 * W + cx[q].i0) * 3, o11 = (cy[q].i1 * W + cx[q].i1) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                pb[q][0][c] = fp[o00 + c], pb[q][1][c] = fp[o01 + c];
                pb[q][2][c] = fp[o10 + c], pb[q][3][c] = fp[o11 + c];
            }
        }
#pragma unroll
        for (int q = 0; q < PPT; ++q) {
            const int u = q / PPG, p = q % PPG;
            const double ax = cx[q].a, ay = cy[q].a;
            const double w00 = (1.0 - ay) * (1.0 - ax), w01 = (1.0 - ay) * ax, w10 = ay * (1.0 - ax), w11 = ay * ax;
            const double m = HAS_W ? (double)vw[q] : 1.0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const unsigned cc = PPG == 4 ? get_byte(cb[u], p * 3 + c) : cb[u][c];
                const double wv = w00 * (double)pb[q][0][c] + w01 * (double)pb[q][1][c] + w10 * (double)pb[q][2][c] +
                                  w11 * (double)pb[q][3][c];
                const double d = (double)cc - wv;
                s1 += valid[u] ? m * fabs(d) : 0.0;
                s2 += valid[u] ? m * (d * d) : 0.0;
            }
            sc += valid[u] ? m : 0.0;
        }
    }
    s1 = block_reduce<REDUCE_SUM, BLOCK>(s1, red);
    s2 = block_reduce<REDUCE_SUM, BLOCK>(s2, red);
    sc = block_reduce<REDUCE_SUM, BLOCK>(sc, red);
    if (tid == 0) {
        double *row = part + ((long)n * rows + blockIdx.x) * 3;
        row[0] = s1, row[1] = s2, row[2] = sc;
    }
}

__global__ void __launch_bounds__(BLOCK)
warp_finish_kernel(const double *__restrict__ part, double *__restrict__ out, int rows, int H, int W) {
    __shared__ double red[BLOCK];
    const int n = blockIdx.x, tid = threadIdx.x;
    const double *row = part + ((long)n * rows + min(tid, rows - 1)) * 3;
    const double p1 = row[0], p2 = row[1], pc = row[2];
    const double s1 = block_reduce<REDUCE_SUM, BLOCK>(tid < rows ? p1 : 0.0, red);
    const double s2 = block_reduce<REDUCE_SUM, BLOCK>(tid < rows ? p2 : 0.0, red);
    const double sc = block_reduce<REDUCE_SUM, BLOCK>(tid < rows ? pc : 0.0, red);
    if (tid == 0) {
        out[(long)n * 3 + 0] = s1 / (127.5 * 3.0 * (double)H * (double)W);
        out[(long)n * 3 + 1] = s2 / (255.0 * 255.0 * 3.0 * sc);
        out[(long)n * 3 + 2] = sc / ((double)H * (double)W);
    }
}

}  // namespace

extern "C" long ir2rgb_warp_error_workspace_bytes(int N, int H, int W) {
    if (!frame_sizes_ok(N, H, W, MIN_SIDE)) return IR2RGB_EINVAL;
    return (long)sizeof(double) * N * 3L * partial_rows((long)H * W, ROW_PIXELS, MAX_ROWS);
}

extern "C" int ir2rgb_warp_error_u8(const uint8_t *prev, const uint8_t *cur, const float *flow, const float *weight,
                                    double *out, void *workspace, long workspace_bytes, int N, int H, int W, void *stream) {
    if (!prev || !cur || !flow || !out || !workspace || !frame_sizes_ok(N, H, W, MIN_SIDE)) return IR2RGB_EINVAL;
    if (workspace_bytes < ir2rgb_warp_error_workspace_bytes(N, H, W)) return IR2RGB_EINVAL;
    if (misaligned(out, 8) || misaligned(workspace, 8) || misaligned(flow, 4) || misaligned(weight, 4)) return IR2RGB_EALIGN;
    const int rows = partial_rows((long)H * W, ROW_PIXELS, MAX_ROWS);
    double *part = static_cast<double *>(workspace);
    hipStream_t s = as_stream(stream);
    const bool wide = W % 4 == 0 && !misaligned(flow, 16) && !misaligned(weight, 16) && !misaligned(cur, 4);
    with_bool(wide, weight != nullptr, [&](auto wd, auto has_w) {
        warp_reduce_kernel<wd.value ? 4 : 1, has_w.value><<<dim3(rows, N), BLOCK, 0, s>>>(prev, cur, flow, weight, part, H, W);
    });
    warp_finish_kernel<<<N, BLOCK, 0, s>>>(part, out, rows, H, W);
    return ir2rgb_launch_status();
}
