// frame_scale.hip -- the loader's Image.resize(..., BICUBIC), crop and flip (reference data/transform.py:64-113) on uint8
// frames that stay on the device, equal to Pillow's 8-bit resampler (Resample.c) byte for byte.
//
// Pillow's resampler is fixed-point.  Per axis, for every output sample xx, the host computes in double a window
// [xmin, xmin + xmax) of source samples and xmax normalised bicubic weights, converted to integers with 22 fraction bits
// (ir2rgb_amd/transform.py: resample_coeffs, Pillow's statement order).  Everything after that is integer arithmetic and
// is what the two kernels below do:
//     out = clamp((2^21 + sum_x px[xmin + x] * k[xx][x]) >> 22, 0, 255)        int32 sum, arithmetic shift
// The horizontal pass runs first and is rounded to uint8, the vertical pass runs on those bytes.
//
//   scale_h_kernel   src [N][Hs][Ws][C] -> workspace [N][rows][Wc][C]: only the source rows [r0, r0 + rows) that the vertical
//                    pass of the kept output rows reads, only the kept columns, already mirrored when flip is set -- so crop
//                    and flip cost nothing and the second pass sees plain rows.  One thread per output pixel (its C bytes
//                    share the weights); consecutive lanes write consecutive pixels.
//   scale_v_kernel   workspace -> dst.  One weight row serves every byte of an output row, so a thread takes 4 consecutive
//                    bytes of the Wc*C-byte row: one dword load per tap, four int32 accumulators, one dword store (rows whose
//                    byte count is a multiple of 4 with 4-byte aligned bases; the scalar form of the same code otherwise).
//                    dst is uint8 [N][Hc][Wc][C] or, through normalise_u8 of u8.h (the one frame_io.hip applies), fp32
//                    [N][C][Hc][Wc].
// A pass whose size does not change gets no tables (bounds == nullptr) and copies; the copy still crops and mirrors.
// Table indices and window positions are clamped to the table / the buffer they read, so a table that does not belong to
// the sizes given cannot make a kernel read outside its operands; writes depend on the sizes alone.
#include "common.h"
#include "u8.h"         // normalise_u8, the bytes of a dword

namespace {

constexpr int PRECISION_BITS = 22;

__device__ __forceinline__ unsigned clip8(int acc) { return (unsigned)min(max(acc >> PRECISION_BITS, 0), 255); }

template <int C>
__global__ void __launch_bounds__(256)
scale_h_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ ws, const int *__restrict__ bounds,
               const int *__restrict__ coef, int ksize, int Hs, int Ws, int r0, int rows, int crop_x, int Wc, int flip,
               long n_items) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n_items; i += (long)gridDim.x * blockDim.x) {
        const int j = (int)(i % Wc);
        const long t = i / Wc;
        const int r = (int)(t % rows);
        const long n = t / rows;
        const int xx = crop_x + (flip ? Wc - 1 - j : j);           // column of the scaled image, < new_w
        const uint8_t *row = src + ((n * Hs + r0 + r) * (long)Ws) * C;
        uint8_t *out = ws + i * C;
        if (bounds == nullptr) {                                    // Ws == new_w: crop and mirror only
#pragma unroll
            for (int c = 0; c < C; ++c) out[c] = row[(long)xx * C + c];
            continue;
        }
        const int xmin = min(max(bounds[2 * xx], 0), Ws - 1);
        const int xmax = min(min(bounds[2 * xx + 1], ksize), Ws - xmin);
        const int *k = coef + (long)xx * ksize;
        int acc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = 1 << (PRECISION_BITS - 1);
        const uint8_t *p = row + (long)xmin * C;
        for (int x = 0; x < xmax; ++x) {
            const int kk = k[x];
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] += (int)p[x * C + c] * kk;
        }
#pragma unroll
        for (int c = 0; c < C; ++c) out[c] = (uint8_t)clip8(acc[c]);
    }
}

// VEC: 4 bytes of a row per thread (Wc * C % 4 == 0, 4-byte aligned bases).  F32: the normalised planar epilogue.
template <int C, bool VEC, bool F32>
__global__ void __launch_bounds__(256)
scale_v_kernel(const uint8_t *__restrict__ ws, void *__restrict__ dst, const int *__restrict__ bounds,
               const int *__restrict__ coef, int ksize, int r0, int rows, int crop_y, int Hc, int Wc, long n_items) {
    constexpr int B = VEC ? 4 : 1;
    const int rowbytes = Wc * C, groups = rowbytes / B;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n_items; i += (long)gridDim.x * blockDim.x) {
        const int g = (int)(i % groups);
        const long t = i / groups;
        const int y = (int)(t % Hc);
        const long n = t / Hc;
        const int yy = crop_y + y;                                  // row of the scaled image
        const uint8_t *col = ws + n * rows * (long)rowbytes + (long)g * B;
        unsigned v[B];
        if (bounds == nullptr) {                                    // Hs == new_h: workspace row y is scaled row yy
            const uint8_t *p = col + (long)min(y, rows - 1) * rowbytes;
            if (VEC) {
                const unsigned w = *reinterpret_cast<const unsigned *>(p);
#pragma unroll
                for (int b = 0; b < B; ++b) v[b] = get_byte(w, b);
            } else {
                v[0] = p[0];
            }
        } else {
            const int ymin = min(max(bounds[2 * yy] - r0, 0), rows - 1);    // first workspace row of the window
            const int ymax = min(min(bounds[2 * yy + 1], ksize), rows - ymin);
            const int *k = coef + (long)yy * ksize;
            int acc[B];
#pragma unroll
            for (int b = 0; b < B; ++b) acc[b] = 1 << (PRECISION_BITS - 1);
            const uint8_t *p = col + (long)ymin * rowbytes;
            for (int x = 0; x < ymax; ++x, p += rowbytes) {
                const int kk = k[x];
                if (VEC) {
                    const unsigned w = *reinterpret_cast<const unsigned *>(p);
#pragma unroll
                    for (int b = 0; b < B; ++b) acc[b] += (int)get_byte(w, b) * kk;
                } else {
                    acc[0] += (int)p[0] * kk;
                }
            }
#pragma unroll
            for (int b = 0; b < B; ++b) v[b] = clip8(acc[b]);
        }
        if (F32) {
            float *out = static_cast<float *>(dst);
#pragma unroll
            for (int b = 0; b < B; ++b) {
                const int byte = g * B + b, x = byte / C, c = byte % C;
                out[((n * C + c) * Hc + y) * (long)Wc + x] = normalise_u8(v[b]);
            }
        } else {
            uint8_t *out = static_cast<uint8_t *>(dst) + (n * Hc + y) * (long)rowbytes + (long)g * B;
            if (VEC) {
                unsigned w = 0;
#pragma unroll
                for (int b = 0; b < B; ++b) w = or_byte(w, b, v[b]);
                *reinterpret_cast<unsigned *>(out) = w;
            } else {
                out[0] = (uint8_t)v[0];
            }
        }
    }
}

// Pillow's precompute_coeffs window of output xx (double, its statement order; no contraction) -> xmin, *xmax
inline int window(int in, int out, int xx, int *xmax) {
#pragma clang fp contract(off)
    const double scale = (double)in / out;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = 2.0 * filterscale;
    const double center = (xx + 0.5) * scale;
    int lo = (int)(center - support + 0.5);
    if (lo < 0) lo = 0;
    int hi = (int)(center + support + 0.5);
    if (hi > in) hi = in;
    *xmax = hi - lo;
    return lo;
}

inline int axis_ksize(int in, int out) {
#pragma clang fp contract(off)
    const double scale = (double)in / out;
    const double support = 2.0 * (scale < 1.0 ? 1.0 : scale);
    return (int)ceil(support) * 2 + 1;
}

struct Geometry {
    int r0, rows;       // source rows the vertical pass of output rows [crop_y, crop_y + Hc) reads
};

// IR2RGB_OK and the row span, or IR2RGB_EINVAL
int geometry(int N, int C, int Hs, int Ws, int new_h, int new_w, int crop_y, int crop_x, int Hc, int Wc, Geometry *g) {
    if (N < 1 || (C != 1 && C != 3) || Hs < 1 || Ws < 1 || new_h < 1 || new_w < 1 || Hc < 1 || Wc < 1 || crop_y < 0 || crop_x < 0)
        return IR2RGB_EINVAL;
    if ((long)crop_y + Hc > new_h || (long)crop_x + Wc > new_w) return IR2RGB_EINVAL;
    const long lim = 0x7fffffffL;
    if ((long)Hs * Ws * C > lim || (long)new_h * new_w * C > lim || (long)Hs * new_w * C > lim) return IR2RGB_EINVAL;
    if (new_h == Hs) {
        g->r0 = crop_y, g->rows = Hc;
    } else {                                                        // both window ends grow with the output index
        int n0, n1;
        g->r0 = window(Hs, new_h, crop_y, &n0);
        const int last = window(Hs, new_h, crop_y + Hc - 1, &n1);
        g->rows = last + n1 - g->r0;
    }
    if (g->rows < 1 || g->r0 < 0 || g->r0 + g->rows > Hs) return IR2RGB_EINVAL;
    return IR2RGB_OK;
}

template <int C>
void launch(const uint8_t *src, void *dst, uint8_t *ws, const int *xb, const int *xc, int xk, const int *yb, const int *yc, int yk,
            int N, int Hs, int Ws, int crop_y, int crop_x, int Hc, int Wc, int flip, bool f32, bool vec, Geometry g,
            hipStream_t s) {
    const long n_h = (long)N * g.rows * Wc;
    scale_h_kernel<C><<<stream_grid(n_h, 256), 256, 0, s>>>(src, ws, xb, xc, xk, Hs, Ws, g.r0, g.rows, crop_x, Wc, flip, n_h);
    const long n_v = (long)N * Hc * (Wc * C / (vec ? 4 : 1));
    with_bool(vec, f32, [&](auto V, auto F32) {
        scale_v_kernel<C, V.value, F32.value>
            <<<stream_grid(n_v, 256), 256, 0, s>>>(ws, dst, yb, yc, yk, g.r0, g.rows, crop_y, Hc, Wc, n_v);
    });
}

}  // namespace

extern "C" long ir2rgb_frame_scale_workspace_bytes(int N, int C, int Hs, int Ws, int new_h, int new_w, int crop_y, int crop_x,
                                                   int Hc, int Wc) {
    Geometry g;
    const int rc = geometry(N, C, Hs, Ws, new_h, new_w, crop_y, crop_x, Hc, Wc, &g);
    if (rc != IR2RGB_OK) return rc;
    return (long)N * g.rows * Wc * C;
}

extern "C" int ir2rgb_frame_scale_u8(const uint8_t *src, void *dst, uint8_t *workspace, long workspace_bytes, const int *xbounds,
                                     const int *xcoef, int xksize, const int *ybounds, const int *ycoef, int yksize, int N, int C,
                                     int Hs, int Ws, int new_h, int new_w, int crop_y, int crop_x, int Hc, int Wc, int flip,
                                     int dst_f32, void *stream) {
    Geometry g;
    const int rc = geometry(N, C, Hs, Ws, new_h, new_w, crop_y, crop_x, Hc, Wc, &g);
    if (rc != IR2RGB_OK) return rc;
    if (!src || !dst || !workspace || (flip != 0 && flip != 1) || (dst_f32 != 0 && dst_f32 != 1)) return IR2RGB_EINVAL;
    if (workspace_bytes < (long)N * g.rows * Wc * C) return IR2RGB_EINVAL;
    // a pass that changes the size needs its tables, with the ksize of that axis; a skipped pass takes none
    const bool need_h = new_w != Ws, need_v = new_h != Hs;
    if (need_h ? (!xbounds || !xcoef || xksize != axis_ksize(Ws, new_w)) : (xbounds || xcoef)) return IR2RGB_EINVAL;
    if (need_v ? (!ybounds || !ycoef || yksize != axis_ksize(Hs, new_h)) : (ybounds || ycoef)) return IR2RGB_EINVAL;
    if (misaligned(xbounds, 4) || misaligned(xcoef, 4) || misaligned(ybounds, 4) || misaligned(ycoef, 4)) return IR2RGB_EALIGN;
    if (dst_f32 && misaligned(dst, 4)) return IR2RGB_EALIGN;
    const bool vec = (Wc * C) % 4 == 0 && !misaligned(workspace, 4) && (dst_f32 || !misaligned(dst, 4));
    hipStream_t s = as_stream(stream);
    auto run = C == 1 ? launch<1> : launch<3>;
    run(src, dst, workspace, xbounds, xcoef, xksize, ybounds, ycoef, yksize, N, Hs, Ws, crop_y, crop_x, Hc, Wc, flip, dst_f32 != 0,
        vec, g, s);
    return ir2rgb_launch_status();
}
