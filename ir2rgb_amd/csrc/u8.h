// u8.h -- fp32 -> 8-bit image values, shared by frame_io.hip (inference) and visuals.hip (training snapshots).
//
// Written with the round-to-nearest intrinsics so that no contraction or reassociation can change the arithmetic:
//   to_u8        trunc(clip((x + 1) / 2 * 255, 0, 255))      numpy: ((x + 1) / 2.0 * 255.0).clip(0, 255).astype(uint8)
//   unit_to_u8   trunc(clip(x * 255, 0, 255))                numpy: (x * 255.0).clip(0, 255).astype(uint8)
// (util.tensor2im with normalize True / False, util/util.py:45-68).  NaN gives 0 in both.
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
