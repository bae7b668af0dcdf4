// u8.h -- the byte vocabulary of the 8-bit image boundary: fp32 <-> 8-bit image values and pixel bytes inside dwords.
// Users: frame_io.hip (inference), frame_scale.hip (the loader's resize), visuals.hip (training snapshots),
// video_metrics.hip and warp_error.hip (the scores), jpeg.hip (the bytes of its bit stream).
//
// Written with the round-to-nearest intrinsics so that no contraction or reassociation can change the arithmetic:
//   to_u8         trunc(clip((x + 1) / 2 * 255, 0, 255))     numpy: ((x + 1) / 2.0 * 255.0).clip(0, 255).astype(uint8)
//   unit_to_u8    trunc(clip(x * 255, 0, 255))               numpy: (x * 255.0).clip(0, 255).astype(uint8)
//   normalise_u8  (float(v) / 255 - 0.5) / 0.5               torch: .float().div(255).sub(0.5).div(0.5)
// (util.tensor2im with normalize True / False, util/util.py:45-68; ToTensor + Normalize(0.5, 0.5), data/transform.py:82-85).
// NaN gives 0 in the first two.
#pragma once
#include <hip/hip_runtime.h>

static __device__ __forceinline__ unsigned to_u8(float x) {
    float v = __fmul_rn(__fdiv_rn(__fadd_rn(x, 1.f), 2.f), 255.f);
    v = fminf(fmaxf(v, 0.f), 255.f);        // (NaN -> 0)
    return (unsigned)(int)v;                 // truncation toward zero, as astype(uint8) on a value in [0, 255]
}

static __device__ __forceinline__ unsigned unit_to_u8(float x) {
    const float v = fminf(fmaxf(__fmul_rn(x, 255.f), 0.f), 255.f);
    return (unsigned)(int)v;
}

static __device__ __forceinline__ float normalise_u8(unsigned v) {
    return __fdiv_rn(__fsub_rn(__fdiv_rn((float)v, 255.f), 0.5f), 0.5f);
}

// byte i (0..3) of a dword as loaded from memory (little endian), and the dword with v or-ed in at byte i
static __device__ __forceinline__ unsigned get_byte(unsigned w, int i) { return (w >> (8 * i)) & 0xffu; }
static __device__ __forceinline__ unsigned or_byte(unsigned w, int i, unsigned v) { return w | v << (8 * i); }
// the same on the bytes of a small dword array: byte i lives in w[i / 4]
static __device__ __forceinline__ unsigned get_byte(const unsigned *w, int i) { return get_byte(w[i >> 2], i & 3); }
static __device__ __forceinline__ void or_byte(unsigned *w, int i, unsigned v) { w[i >> 2] = or_byte(w[i >> 2], i & 3, v); }

// the four floats of a 16-byte load
static __device__ __forceinline__ void unpack4(float4 t, float *f) { f[0] = t.x, f[1] = t.y, f[2] = t.z, f[3] = t.w; }
