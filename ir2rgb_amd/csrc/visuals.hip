// visuals.hip -- training snapshots: what the reference shows of a run every display_freq sequences, as 8-bit panels
// composed on the device.
//
// The reference (train_vid2vid.py:131-136, util.save_all_tensors, util/util.py:13-104) takes nine whole fp32 tensors to
// the host and converts them there with numpy and cv2.  Here one call turns up to 16 fp32 NCHW planes the trainer
// already holds into one uint8 [P][H][W][3] stack; only those bytes leave the device.  Panel kinds:
//   IMAGE_NORM  tensor2im(x)                    to_u8 of u8.h, C = 1 or 3 (one channel is written three times)
//   IMAGE_UNIT  tensor2im(x, normalize=False)   unit_to_u8 of u8.h
//   FLOW        tensor2flow(x), C = 2: hue = direction, value = magnitude scaled to the panel's own [min, max]
//
// The flow coding in two stages.  Floats to bytes (fp32, round-to-nearest intrinsics, no contraction):
//   mag = sqrt(u*u + v*v);  [mn, mx] = min / max of mag over the panel (fminf / fmaxf: NaN magnitudes are ignored)
//   Hb  = trunc(ang * 90 / pi) mod 180, ang = atan2(v, u) in [0, 2 pi).  Evaluated by octants -- atan of
//         min(|u|,|v|) / max(|u|,|v|) in [0, pi/4], reflected with the exact constants 45, 90, 180 -- so that the axis
//         directions give exactly 0, 45, 90, 135 whatever the rounding of pi
//   Vb  = trunc((mag - mn) * 255 / (mx - mn)), 0 for every pixel when mx == mn and for a NaN magnitude;  S = 255
// Bytes to RGB (integers only, exact): i = Hb / 30, r = Hb % 30, t = (2 Vb r + 30) / 60 rising, q = (2 Vb (30 - r) + 30) / 60
// falling, p = 0, and the six-sector assignment of (V, t, p, q) to R, G, B.
//
// Two launches when a flow panel is present, one otherwise.  visuals_minmax_kernel: up to 256 workgroups per flow panel,
// each writes one (min, max) row of the workspace -- min and max do not depend on the order, so the result is
// bit-reproducible.  visuals_panel_kernel: a workgroup belongs to ONE panel (blockIdx.x / blocks_per_panel), so kind and
// channel count are wave-uniform and no access spans two panels; the workgroups of a flow panel first fold that panel's
// rows.  Both are HBM-bound grid-stride loops with 64-bit offsets: at 512x1024 with the nine panels of a training run
// 21 fp32 planes (44 MB) are read for the panels, 4 of them (8 MB) once more for the ranges, 14 MB written.  Rows whose
// width is a multiple of 4 with 16-byte aligned sources and a 4-byte aligned stack take 16-byte loads and write 4 pixels
// as three dwords (as frame_finish_kernel of frame_io.hip does), everything else the scalar form of the same code.
// The panel table travels by value in the kernel's argument segment: no device-side table, no upload.
#include <math.h>

#include "common.h"
#include "reduce.h"     // partial_rows
#include "u8.h"         // to_u8, unit_to_u8, the bytes of a pixel group

namespace {

struct PanelTable {
    const float *src[IR2RGB_VISUALS_MAX_PANELS];
    int kind[IR2RGB_VISUALS_MAX_PANELS];
    int channels[IR2RGB_VISUALS_MAX_PANELS];
    int flow_slot[IR2RGB_VISUALS_MAX_PANELS];      // panel -> its row block in the workspace (flow panels only)
    int flow_panel[IR2RGB_VISUALS_MAX_PANELS];     // the inverse: flow panel f -> panel index
};

__device__ __forceinline__ float flow_mag(float u, float v) {
    return __fsqrt_rn(__fadd_rn(__fmul_rn(u, u), __fmul_rn(v, v)));
}

// min and max over the workgroup (256 threads = 4 waves), handed to every thread
__device__ __forceinline__ void block_minmax(float &mn, float &mx) {
    __shared__ float part[2][4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o));
        mx = fmaxf(mx, __shfl_xor(mx, o));
    }
    if ((threadIdx.x & 63) == 0) part[0][threadIdx.x >> 6] = mn, part[1][threadIdx.x >> 6] = mx;
    __syncthreads();
    mn = fminf(fminf(part[0][0], part[0][1]), fminf(part[0][2], part[0][3]));
    mx = fmaxf(fmaxf(part[1][0], part[1][1]), fmaxf(part[1][2], part[1][3]));
}

// workgroup b of `rows` of flow panel f: its (min, max) of the magnitude -> workspace row [f][b]
template <bool VEC>
__global__ void __launch_bounds__(256)
visuals_minmax_kernel(PanelTable tab, float *__restrict__ ws, int rows, long hw) {
    const int f = blockIdx.x / rows, b = blockIdx.x % rows;
    const float *__restrict__ u = tab.src[tab.flow_panel[f]];
    const float *__restrict__ v = u + hw;
    float mn = INFINITY, mx = -INFINITY;
    const long n = VEC ? hw >> 2 : hw;
    for (long i = b * 256L + threadIdx.x; i < n; i += rows * 256L) {
        if (VEC) {
            const float4 a = *reinterpret_cast<const float4 *>(u + (i << 2)), c = *reinterpret_cast<const float4 *>(v + (i << 2));
            const float m[4] = {flow_mag(a.x, c.x), flow_mag(a.y, c.y), flow_mag(a.z, c.z), flow_mag(a.w, c.w)};
#pragma unroll
            for (int k = 0; k < 4; ++k) mn = fminf(mn, m[k]), mx = fmaxf(mx, m[k]);
        } else {
            const float m = flow_mag(u[i], v[i]);
            mn = fminf(mn, m), mx = fmaxf(mx, m);
        }
    }
    block_minmax(mn, mx);
    if (threadIdx.x == 0) ws[2 * ((long)f * rows + b)] = mn, ws[2 * ((long)f * rows + b) + 1] = mx;
}

// one flow vector -> its three bytes, R | G << 8 | B << 16
__device__ __forceinline__ unsigned flow_rgb(float u, float v, float mn, float range) {
    const float au = fabsf(u), av = fabsf(v), lo = fminf(au, av), hi = fmaxf(au, av);
    float t = hi > 0.f ? __fmul_rn(atanf(__fdiv_rn(lo, hi)), 28.6478897565411604f) : 0.f;      // 90 / pi: [0, 22.5]
    if (av > au) t = __fsub_rn(45.f, t);
    if (u < 0.f) t = __fsub_rn(90.f, t);
    if (v < 0.f) t = __fsub_rn(180.f, t);
    int hb = (int)fminf(fmaxf(t, 0.f), 180.f);          // (NaN -> 0)
    if (hb >= 180) hb -= 180;
    const float val = range > 0.f ? __fdiv_rn(__fmul_rn(__fsub_rn(flow_mag(u, v), mn), 255.f), range) : 0.f;
    const int vb = (int)fminf(fmaxf(val, 0.f), 255.f);  // (NaN -> 0)
    const int i = hb / 30, r = hb - 30 * i;
    const unsigned up = (unsigned)(2 * vb * r + 30) / 60u, dn = (unsigned)(2 * vb * (30 - r) + 30) / 60u, V = (unsigned)vb;
    switch (i) {
    case 0: return V | up << 8;
    case 1: return dn | V << 8;
    case 2: return V << 8 | up << 16;
    case 3: return dn << 8 | V << 16;
    case 4: return up | V << 16;
    default: return V | dn << 16;
    }
}

// the three bytes of pixel e of a panel.  KIND, C: the panel's; FLOW reads mn and range = mx - mn
template <int KIND, int C>
__device__ __forceinline__ unsigned pixel_rgb(const float (&x)[3], float mn, float range) {
    if (KIND == IR2RGB_PANEL_FLOW) return flow_rgb(x[0], x[1], mn, range);
    unsigned b[3];
#pragma unroll
    for (int c = 0; c < C; ++c) b[c] = KIND == IR2RGB_PANEL_IMAGE_NORM ? to_u8(x[c]) : unit_to_u8(x[c]);
    return C == 1 ? b[0] * 0x010101u : (b[0] | b[1] << 8 | b[2] << 16);
}

template <int KIND, int C, bool VEC>
__device__ __forceinline__ void run_panel(const float *__restrict__ src, uint8_t *__restrict__ dst, long hw, int b, int bpp,
                                          float mn, float range) {
    const long n = VEC ? hw >> 2 : hw;
    for (long i = b * 256L + threadIdx.x; i < n; i += bpp * 256L) {
        if (VEC) {
            const long e = i << 2;          // 4 pixels (hw % 4 == 0)
            float x[4][3];
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float4 t = *reinterpret_cast<const float4 *>(src + c * hw + e);
                x[0][c] = t.x, x[1][c] = t.y, x[2][c] = t.z, x[3][c] = t.w;
            }
            unsigned w[3] = {0u, 0u, 0u};
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const unsigned rgb = pixel_rgb<KIND, C>(x[p], mn, range);
#pragma unroll
                for (int c = 0; c < 3; ++c) or_byte(w, p * 3 + c, get_byte(rgb, c));
            }
            unsigned *out = reinterpret_cast<unsigned *>(dst + e * 3);
#pragma unroll
            for (int k = 0; k < 3; ++k) out[k] = w[k];
        } else {
            float x[3];
#pragma unroll
            for (int c = 0; c < C; ++c) x[c] = src[c * hw + i];
            const unsigned rgb = pixel_rgb<KIND, C>(x, mn, range);
            dst[i * 3] = (uint8_t)rgb, dst[i * 3 + 1] = (uint8_t)(rgb >> 8), dst[i * 3 + 2] = (uint8_t)(rgb >> 16);
        }
    }
}

// workgroup b of `bpp` of panel p
template <bool VEC>
__global__ void __launch_bounds__(256)
visuals_panel_kernel(PanelTable tab, const float *__restrict__ ws, int rows, uint8_t *__restrict__ out, long hw, int bpp) {
    const int p = blockIdx.x / bpp, b = blockIdx.x % bpp;
    const float *__restrict__ src = tab.src[p];
    const int kind = tab.kind[p], ch = tab.channels[p];
    uint8_t *__restrict__ dst = out + (long)p * hw * 3;
    if (kind == IR2RGB_PANEL_FLOW) {
        float mn = INFINITY, mx = -INFINITY;
        if ((int)threadIdx.x < rows) {      // (rows <= 256)
            const float *row = ws + 2 * ((long)tab.flow_slot[p] * rows + threadIdx.x);
            mn = row[0], mx = row[1];
        }
        block_minmax(mn, mx);
        run_panel<IR2RGB_PANEL_FLOW, 2, VEC>(src, dst, hw, b, bpp, mn, mx > mn ? __fsub_rn(mx, mn) : 0.f);
    } else if (kind == IR2RGB_PANEL_IMAGE_NORM) {
        if (ch == 3) run_panel<IR2RGB_PANEL_IMAGE_NORM, 3, VEC>(src, dst, hw, b, bpp, 0.f, 0.f);
        else run_panel<IR2RGB_PANEL_IMAGE_NORM, 1, VEC>(src, dst, hw, b, bpp, 0.f, 0.f);
    } else {
        if (ch == 3) run_panel<IR2RGB_PANEL_IMAGE_UNIT, 3, VEC>(src, dst, hw, b, bpp, 0.f, 0.f);
        else run_panel<IR2RGB_PANEL_IMAGE_UNIT, 1, VEC>(src, dst, hw, b, bpp, 0.f, 0.f);
    }
}

// (min, max) rows per flow panel: one per workgroup of visuals_minmax_kernel, a workgroup per 1024 pixels, at most 256
inline int minmax_rows(long hw) { return partial_rows(hw, 1024, 256); }

}  // namespace

extern "C" long ir2rgb_visuals_workspace_bytes(int n_flow_panels, int H, int W) {
    if (n_flow_panels < 0 || n_flow_panels > IR2RGB_VISUALS_MAX_PANELS || H < 1 || W < 1 || (long)H * W * 3 > 0x7fffffffL)
        return IR2RGB_EINVAL;
    return (long)n_flow_panels * minmax_rows((long)H * W) * 2 * (long)sizeof(float);
}

extern "C" int ir2rgb_visuals_u8(const ir2rgb_panel *panels, int n, int H, int W, float *workspace, uint8_t *out, void *stream) {
    if (!panels || !out || n < 1 || n > IR2RGB_VISUALS_MAX_PANELS || H < 1 || W < 1 || (long)H * W * 3 > 0x7fffffffL)
        return IR2RGB_EINVAL;
    PanelTable tab{};
    int n_flow = 0;
    bool vec = W % 4 == 0 && !misaligned(out, 4);
    for (int p = 0; p < n; ++p) {
        const ir2rgb_panel &q = panels[p];
        const bool image = q.kind == IR2RGB_PANEL_IMAGE_NORM || q.kind == IR2RGB_PANEL_IMAGE_UNIT;
        if (!q.src || !(image ? q.channels == 1 || q.channels == 3 : q.kind == IR2RGB_PANEL_FLOW && q.channels == 2))
            return IR2RGB_EINVAL;
        tab.src[p] = q.src, tab.kind[p] = q.kind, tab.channels[p] = q.channels;
        if (q.kind == IR2RGB_PANEL_FLOW) tab.flow_slot[p] = n_flow, tab.flow_panel[n_flow++] = p;
        vec = vec && !misaligned(q.src, 16);
    }
    if (n_flow && !workspace) return IR2RGB_EINVAL;
    for (int p = 0; p < n; ++p)
        if (misaligned(panels[p].src, 4)) return IR2RGB_EALIGN;
    if (misaligned(workspace, 4)) return IR2RGB_EALIGN;
    const long hw = (long)H * W;
    const int rows = minmax_rows(hw);
    hipStream_t s = as_stream(stream);
    // workgroups per panel: one per 256 work items, the whole grid within what stream_grid hands a streaming kernel
    int bpp = stream_grid(vec ? hw >> 2 : hw, 256);
    if (bpp > 2048 / n) bpp = 2048 / n;
    with_bool(vec, [&](auto V) {
        if (n_flow) visuals_minmax_kernel<V.value><<<n_flow * rows, 256, 0, s>>>(tab, workspace, rows, hw);
        visuals_panel_kernel<V.value><<<n * bpp, 256, 0, s>>>(tab, workspace, rows, out, hw, bpp);
    });
    return ir2rgb_launch_status();
}
