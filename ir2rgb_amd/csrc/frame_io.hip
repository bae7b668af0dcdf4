// frame_io.hip -- the 8-bit image boundary and the device-resident recurrence state of frame-by-frame inference.
//
// One inference step of the reference (models/generator.py:184-235, test_vid2vid.py:36-60) wraps the generator forward in
// torch / numpy glue: transforms.ToTensor + Normalize(0.5, 0.5) on the loaded frame (data/transform.py:82-85), build_pyr on
// the whole input window (base_model.py:64-82), torch.cat([prev[1:], fake_B]) per scale (generator.py:214) and
// util.tensor2im on the result (util/util.py:45-67).  The two kernels below do that work on histories that stay on the
// device: each moves a history one slot down IN PLACE (one thread reads slot k+1 and writes slot k at the same element
// index, so no second buffer and no ordering between threads is needed) and fills the newest slot.
//
// Both are HBM-bound: per 512x1024 3-channel frame ir2rgb_frame_push_u8 reads 1.5 MB of bytes and moves the fp32
// histories, ir2rgb_frame_finish_u8 reads 6 MB of fp32 and writes 1.5 MB of bytes beside the history.  Rows whose width
// is a multiple of 4 go through 16-byte fp32 loads / stores (4 pixels per thread; their 4*C bytes as C dword accesses);
// other widths, and pooled rows whose width is not a multiple of 4, take the scalar-width form of the same code.
//
// Arithmetic is written with the round-to-nearest intrinsics so that no contraction or reassociation can change it:
//   normalise   (float(v) / 255 - 0.5) / 0.5                 torch: .float().div(255).sub(0.5).div(0.5)
//   to 8 bit    trunc(clip((x + 1) / 2 * 255, 0, 255))       numpy: ((x + 1) / 2.0 * 255.0).clip(0, 255).astype(uint8)
//   pooling     the statement order of avgpool3s2_fwd_kernel (pointwise.hip): rows outer, columns inner, one division
#include "common.h"
#include "u8.h"         // to_u8, normalise_u8, the bytes of a pixel group

namespace {

// history [T][plane] -> slots 1..T-1 move to 0..T-2 at element(s) e, the newest slot receives v
template <typename V>
__device__ __forceinline__ void shift_in(float *hist, int T, long plane, long e, V v) {
    V *p = reinterpret_cast<V *>(hist + e);
    const long step = plane / (long)(sizeof(V) / sizeof(float));
    for (int k = 0; k + 1 < T; ++k) p[k * step] = p[(k + 1) * step];
    p[(long)(T - 1) * step] = v;
}

// the new frame's normalised value at (c, y, x): from the interleaved bytes or from an fp32 [C][H][W] frame
template <int C, bool F32>
__device__ __forceinline__ float pixel(const void *frame, int H, int W, int c, int y, int x) {
    if (F32) return static_cast<const float *>(frame)[((long)c * H + y) * W + x];
    return normalise_u8(static_cast<const uint8_t *>(frame)[((long)y * W + x) * C + c]);
}

template <int C, bool F32>
__device__ __forceinline__ float pooled(const void *frame, int H, int W, int c, int oy, int ox) {
    const int y0 = max(2 * oy - 1, 0), y1 = min(2 * oy + 1, H - 1), x0 = max(2 * ox - 1, 0), x1 = min(2 * ox + 1, W - 1);
    float s = 0.f;
    for (int yy = y0; yy <= y1; ++yy)
        for (int xx = x0; xx <= x1; ++xx) s += pixel<C, F32>(frame, H, W, c, yy, xx);
    return s / (float)((y1 - y0 + 1) * (x1 - x0 + 1));
}

// VF: the full level runs 4 pixels per thread (W % 4 == 0); VP: the pooled level runs 4 outputs per thread (Wo % 4 == 0).
// Work items [0, n_full) are pixel groups of the full level (all C channels each), [n_full, n_full + n_pool) are
// (channel, output group) pairs of the pooled level.
template <int C, bool F32, bool VF, bool VP>
__global__ void __launch_bounds__(256)
frame_push_kernel(const void *__restrict__ frame, float *__restrict__ hist0, float *__restrict__ hist1, int T, int H, int W,
                  int Ho, int Wo, long n_full, long n_pool) {
    const long plane0 = (long)C * H * W, plane1 = (long)C * Ho * Wo;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n_full + n_pool; i += (long)gridDim.x * blockDim.x) {
        if (i < n_full) {
            if (VF) {
                const int wq = W >> 2;
                const int y = (int)(i / wq), x = (int)(i % wq) << 2;
                float v[C][4];
                if (F32) {
#pragma unroll
                    for (int c = 0; c < C; ++c)
                        unpack4(*reinterpret_cast<const float4 *>(static_cast<const float *>(frame) + ((long)c * H + y) * W + x), v[c]);
                } else {
                    unsigned b[C];      // 4 pixels x C channels = C dwords of interleaved bytes
                    const unsigned *src = reinterpret_cast<const unsigned *>(static_cast<const uint8_t *>(frame) + ((long)y * W + x) * C);
#pragma unroll
                    for (int k = 0; k < C; ++k) b[k] = src[k];
#pragma unroll
                    for (int p = 0; p < 4; ++p)
#pragma unroll
                        for (int c = 0; c < C; ++c) v[c][p] = normalise_u8(get_byte(b, p * C + c));
                }
#pragma unroll
                for (int c = 0; c < C; ++c)
                    shift_in(hist0, T, plane0, ((long)c * H + y) * W + x, make_float4(v[c][0], v[c][1], v[c][2], v[c][3]));
            } else {
                const int y = (int)(i / W), x = (int)(i % W);
#pragma unroll
                for (int c = 0; c < C; ++c)
                    shift_in(hist0, T, plane0, ((long)c * H + y) * W + x, pixel<C, F32>(frame, H, W, c, y, x));
            }
        } else {
            long j = i - n_full;
            const int wg = VP ? (Wo >> 2) : Wo;
            const int g = (int)(j % wg);
            j /= wg;
            const int oy = (int)(j % Ho), c = (int)(j / Ho);
            if (VP) {
                const int ox = g << 2;
                const float4 t = make_float4(pooled<C, F32>(frame, H, W, c, oy, ox), pooled<C, F32>(frame, H, W, c, oy, ox + 1),
                                             pooled<C, F32>(frame, H, W, c, oy, ox + 2), pooled<C, F32>(frame, H, W, c, oy, ox + 3));
                shift_in(hist1, T, plane1, ((long)c * Ho + oy) * Wo + ox, t);
            } else {
                shift_in(hist1, T, plane1, ((long)c * Ho + oy) * Wo + g, pooled<C, F32>(frame, H, W, c, oy, g));
            }
        }
    }
}

template <bool VEC>
__global__ void __launch_bounds__(256)
frame_finish_kernel(const float *__restrict__ x, float *__restrict__ hist, uint8_t *__restrict__ img, int T, int H, int W, long n) {
    const long hw = (long)H * W, plane = 3 * hw;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        if (VEC) {
            const long e = i << 2;          // 4 pixels of one row (W % 4 == 0)
            float v[3][4];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float4 t = *reinterpret_cast<const float4 *>(x + c * hw + e);
                unpack4(t, v[c]);
                shift_in(hist, T, plane, c * hw + e, t);
            }
            if (img) {
                unsigned b[3] = {0u, 0u, 0u};
#pragma unroll
                for (int p = 0; p < 4; ++p)
#pragma unroll
                    for (int c = 0; c < 3; ++c) or_byte(b, p * 3 + c, to_u8(v[c][p]));
                unsigned *dst = reinterpret_cast<unsigned *>(img + e * 3);
#pragma unroll
                for (int k = 0; k < 3; ++k) dst[k] = b[k];
            }
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float t = x[c * hw + i];
                shift_in(hist, T, plane, c * hw + i, t);
                if (img) img[i * 3 + c] = (uint8_t)to_u8(t);
            }
        }
    }
}

template <int C, bool F32>
void launch_push(const void *frame, float *hist0, float *hist1, int T, int H, int W, int Ho, int Wo, bool vf, bool vp, hipStream_t s) {
    const long n_full = vf ? (long)H * (W >> 2) : (long)H * W;
    const long n_pool = hist1 ? (long)C * Ho * (vp ? (Wo >> 2) : Wo) : 0;
    const int grid = stream_grid(n_full + n_pool, 256);
    // vp implies vf, so the pair (false, true) never arrives: it is mapped onto <false, false> and no such kernel is built
    with_bool(vf, vp, [&](auto VF, auto VP) {
        frame_push_kernel<C, F32, VF.value, VF.value && VP.value>
            <<<grid, 256, 0, s>>>(frame, hist0, hist1, T, H, W, Ho, Wo, n_full, n_pool);
    });
}

}  // namespace

extern "C" int ir2rgb_frame_push_u8(const void *frame, float *hist0, float *hist1, int T, int C, int H, int W, int src_f32,
                                    void *stream) {
    if (!frame || !hist0 || T < 1 || (C != 1 && C != 3) || H < 1 || W < 1 || (src_f32 != 0 && src_f32 != 1)) return IR2RGB_EINVAL;
    if ((long)C * H * W > 0x7fffffffL) return IR2RGB_EINVAL;
    if (misaligned(hist0, 4) || misaligned(hist1, 4) || (src_f32 && misaligned(frame, 4))) return IR2RGB_EALIGN;
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    // 16-byte accesses need rows that are multiples of 4 floats and 16-byte bases (the byte frame: 4*C bytes per group -> dword)
    const bool vf = W % 4 == 0 && !misaligned(hist0, 16) && !misaligned(frame, src_f32 ? 16 : 4);
    const bool vp = vf && hist1 && Wo % 4 == 0 && !misaligned(hist1, 16);
    hipStream_t s = as_stream(stream);
    with_bool(src_f32 != 0, [&](auto f32) {
        (C == 1 ? launch_push<1, f32.value> : launch_push<3, f32.value>)(frame, hist0, hist1, T, H, W, Ho, Wo, vf, vp, s);
    });
    return ir2rgb_launch_status();
}

extern "C" int ir2rgb_frame_finish_u8(const float *x, float *hist, uint8_t *img_u8, int T, int H, int W, void *stream) {
    if (!x || !hist || T < 1 || H < 1 || W < 1 || (long)H * W * 3 > 0x7fffffffL) return IR2RGB_EINVAL;
    if (misaligned(x, 4) || misaligned(hist, 4)) return IR2RGB_EALIGN;
    const bool vec = W % 4 == 0 && !misaligned(x, 16) && !misaligned(hist, 16) && !misaligned(img_u8, 4);
    const long n = vec ? ((long)H * W) >> 2 : (long)H * W;
    hipStream_t s = as_stream(stream);
    with_bool(vec, [&](auto V) { frame_finish_kernel<V.value><<<stream_grid(n, 256), 256, 0, s>>>(x, hist, img_u8, T, H, W, n); });
    return ir2rgb_launch_status();
}
