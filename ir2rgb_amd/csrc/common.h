// common.h -- shared helpers for the gfx950 kernels of libir2rgb_hip.so
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <type_traits>

#include "../../include/ir2rgb_hip.h"

#define IR2RGB_WAVE 64

static inline int ir2rgb_launch_status() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? IR2RGB_OK : (int)e;
}

static inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

// Calls f with the half element type (checked by the caller) as a compile-time constant, so that a launch site
// names its kernel and its argument list once:  with_dtype(dtype, [&](auto dt) { K<dt.value><<<...>>>(...); });
template <class F> static inline void with_dtype(int dtype, F &&f) {
    if (dtype == IR2RGB_BF16) f(std::integral_constant<int, IR2RGB_BF16>{});
    else f(std::integral_constant<int, IR2RGB_F16>{});
}

// The same for run-time flags that select a kernel form:  with_bool(vec, [&](auto v) { K<v.value><<<...>>>(...); });
// f is instantiated for every value (all four pairs in the two-flag form).  A launch site whose kernel has fewer forms maps
// the pairs it never takes onto one it has, in the template arguments, so that no further kernel is compiled.
template <class F> static inline void with_bool(bool flag, F &&f) {
    if (flag) f(std::true_type{});
    else f(std::false_type{});
}
template <class F> static inline void with_bool(bool a, bool b, F &&f) {
    with_bool(a, [&](auto ca) { with_bool(b, [&](auto cb) { f(ca, cb); }); });
}

// An integer environment switch (IR2RGB_CONV3X3P, IR2RGB_CONV3X3P_SPLIT, IR2RGB_CONV_DOT, IR2RGB_CONV_HALF_TILE): unset = dflt.  Callers keep
// the value in a function-local static: the environment is read once per process.
static inline int env_switch(const char *name, int dflt) {
    const char *e = getenv(name);
    return e ? atoi(e) : dflt;
}

// What every convolution plan resolves first: the dense defaults of the channel-slice views, the byte extents of X and
// of a half-precision Y (buffer resources want them below 2^31) and whether dtype is one of the two half types.
struct ConvView {
    int ldx, ldy;
    long x_bytes, y_bytes;
    bool half;
};
static inline ConvView conv_view(const ir2rgb_conv_desc *d) {
    ConvView v{};
    if (!d) return v;
    v.ldx = d->ldx > 0 ? d->ldx : d->Cin; v.ldy = d->ldy > 0 ? d->ldy : d->Cout;
    // (nothing of d is validated yet: the product of five ints fits 128 bits and is clamped to what a long holds)
    auto bytes = [](int n, int h, int w, int ld) {
        const __int128 b = (__int128)n * h * w * ld * 2, lim = (__int128)1 << 62;
        return (long)(b > lim ? lim : b < -lim ? -lim : b);
    };
    v.x_bytes = bytes(d->N, d->Hin, d->Win, v.ldx); v.y_bytes = bytes(d->N, d->Hout, d->Wout, v.ldy);
    v.half = d->dtype == IR2RGB_BF16 || d->dtype == IR2RGB_F16;
    return v;
}

static inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// p is off an a-byte boundary (a a power of two); NULL is aligned
static inline bool misaligned(const void *p, unsigned a) { return ((uintptr_t)p & (a - 1)) != 0; }

// grid size for HBM-bound grid-stride kernels: enough blocks to fill 256 CUs x 8 blocks.
static inline int stream_grid(long work_items, int block) {
    long g = (work_items + block - 1) / block;
    if (g > 2048) g = 2048;
    if (g < 1) g = 1;
    return (int)g;
}

// Exact unsigned 32-bit division by a launch-time constant d >= 2 (branch-free round-up method):
//   q = (t + ((n - t) >> 1)) >> sh,  t = umulhi(m, n).  d == 1 is encoded as m = 0, sh = 32 (q = n).
struct FastDiv {
    unsigned m, sh;
};
static inline FastDiv make_fastdiv(unsigned d) {
    FastDiv f;
    if (d <= 1) { f.m = 0; f.sh = 32; return f; }
    unsigned s = 0;
    while ((1ull << s) < d) ++s;  // ceil(log2 d) >= 1
    f.m = (unsigned)((((1ull << 32) * ((1ull << s) - d)) / d) + 1);
    f.sh = s - 1;
    return f;
}
#ifdef __HIPCC__
// half <-> float with the element type as a run-time value (the pointwise kernels)
static __device__ __forceinline__ float h2f(uint16_t h, int dt) {
    if (dt == IR2RGB_BF16) return __uint_as_float(((uint32_t)h) << 16);
    _Float16 v = __builtin_bit_cast(_Float16, h);
    return (float)v;
}
static __device__ __forceinline__ uint16_t f2h(float f, int dt) {
    if (dt == IR2RGB_BF16) { __bf16 h = (__bf16)f; return __builtin_bit_cast(uint16_t, h); }
    _Float16 h = (_Float16)f;
    return __builtin_bit_cast(uint16_t, h);
}

// 8 halfs of a 16-byte lane <-> 8 floats (the NHWC side of the HBM-bound kernels)
__device__ __forceinline__ void unpack8(const uint4 &v, float *f, int dt) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        f[2 * j] = h2f((uint16_t)(w[j] & 0xffff), dt);
        f[2 * j + 1] = h2f((uint16_t)(w[j] >> 16), dt);
    }
}
__device__ __forceinline__ uint4 pack8(const float *f, int dt) {
    uint32_t w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] = (uint32_t)f2h(f[2 * j], dt) | ((uint32_t)f2h(f[2 * j + 1], dt) << 16);
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// g' = gz * act'(pre) where pre = y*scale+shift (BN output) or y itself (scale == nullptr)
__device__ __forceinline__ float act_grad(float g, float pre, int act) {
    if (act == 1) return pre > 0.f ? g : 0.f;
    if (act == 2) return pre > 0.f ? g : 0.2f * g;
    return g;
}

__device__ __forceinline__ unsigned fdiv(unsigned n, FastDiv f) {
    if (f.sh == 32) return n;
    const unsigned t = __umulhi(f.m, n);
    return (t + ((n - t) >> 1)) >> f.sh;
}

// inf or NaN: decided from the value's exponent field (3e38 is finite although its square is not a float)
__device__ __forceinline__ bool nonfinite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

// fixed-order sum over the 64 lanes of a wave (lane 0 holds the total)
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
    return v;
}

// sum over the 16 lanes of a DPP row (all lanes end with the row total): two quad permutes, a
// half-row mirror and a row mirror, each folded into the v_add as a DPP operand.
__device__ __forceinline__ float row16_sum(float v) {
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));   // quad_perm [1,0,3,2]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));   // quad_perm [2,3,0,1]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));  // row_half_mirror
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true));  // row_mirror
    return v;
}

// ---- shared by the MFMA / LDS-DMA kernels (every .hip file is its own translation unit) ----
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((address_space(3))) void *lptr_t;
typedef __amdgpu_buffer_rsrc_t rsrc_t;

// element type of the half-precision operands: MFMA fragment, the 16x16x32 MFMA, fp32 -> half conversion
template <int DT> struct Half;
template <> struct Half<IR2RGB_BF16> {
    typedef bf16x8 frag;
    static __device__ __forceinline__ f32x4 mfma(frag a, frag b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ uint16_t cvt(float f) {
        __bf16 h = (__bf16)f;
        return __builtin_bit_cast(uint16_t, h);
    }
};
template <> struct Half<IR2RGB_F16> {
    typedef f16x8 frag;
    static __device__ __forceinline__ f32x4 mfma(frag a, frag b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ uint16_t cvt(float f) {
        _Float16 h = (_Float16)f;
        return __builtin_bit_cast(uint16_t, h);
    }
};

// Buffer-addressed LDS-DMA: 16 B per lane from (SGPR base + per-lane 32-bit byte offset + scalar byte
// offset) to LDS at wave-uniform base + lane * 16.  The per-lane offset is range-checked against the
// resource extent and out-of-range lanes deliver ZEROS: zero padding costs no instruction, and the
// scalar K offset rides in an SGPR, so a K-step's staging issues no VALU address arithmetic at all.
#define IR2RGB_OOB 0x80000000u  // per-lane offset past any extent (extents are < 2^31)
__device__ __forceinline__ rsrc_t make_rsrc(const void *p, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p), 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ void lds_dma16(rsrc_t r, unsigned voff, unsigned soff, lptr_t dst_wave_base) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(r, dst_wave_base, 16, voff, soff, 0, 0);
}
__device__ __forceinline__ void lds_dma16(rsrc_t r, unsigned voff, unsigned soff, void *dst_wave_base) {
    lds_dma16(r, voff, soff, (lptr_t)dst_wave_base);
}

// index of a reflection-padded coordinate (no edge repeat)
__device__ __forceinline__ int reflect(int v, int n) {
    v = v < 0 ? -v : v;
    return v >= n ? 2 * n - 2 - v : v;
}
#endif
