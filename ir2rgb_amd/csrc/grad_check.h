// grad_check.h -- what loss_scale.hip (the loss-scaled step) and grad_guard.hip (the guarded step) share: one read of a
// gradient table that decides "finite?" and sums the squares.  grad_check_kernel writes one row per (tensor, chunk)
// workgroup, and each file's finish kernel (one workgroup of CHECK_FINISH_THREADS lanes) sums the rows in the same order and
// applies its rule.  Every sum is in double in a fixed order (thread, wave, workgroup, row), nothing is atomic, loads are
// unconditional from clamped indices and masked afterwards (DESIGN, "Small kernels are latency-shaped").
#pragma once
#include "adam.h"

struct CheckRow {
    double sumsq;
    float nonfinite, reserved;
};
static_assert(sizeof(CheckRow) == 16, "one 16-byte load per partial row");

#define CHECK_FINISH_THREADS 1024

// inf or NaN: decided from the value's exponent field (3e38 is finite although its square is not a float)
__device__ __forceinline__ bool nonfinite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

// fixed-order sum over the 64 lanes of a wave (lane 0 holds the total)
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
    return v;
}

// (static: one definition in this header, compiled into each object that launches it)
static __global__ void __launch_bounds__(256)
grad_check_kernel(const AdamTensor *__restrict__ table, const int2 *__restrict__ blocks, CheckRow *__restrict__ partial) {
    const int2 tb = blocks[blockIdx.x];
    const AdamTensor t = table[tb.x];
    const long e0 = (long)tb.y * ADAM_CHUNK;
    const long e1 = min(t.n, e0 + ADAM_CHUNK);
    // the same three cases as adam_kernel, so that the 16-byte path is taken exactly where the step takes it
    const bool vec = ((((uintptr_t)t.p | (uintptr_t)t.g | (uintptr_t)t.m | (uintptr_t)t.v) & 15) == 0);
    double acc = 0.0;
    bool bad = false;
    auto take = [&](float g) { bad |= nonfinite(g); acc += (double)g * (double)g; };
    if (vec && e1 - e0 == ADAM_CHUNK) {
        typedef float vf4 __attribute__((ext_vector_type(4)));
        typedef __attribute__((address_space(1))) vf4 gf4;
        const gf4 *g4 = (const gf4 *)(uintptr_t)t.g;
        const long q0 = (e0 >> 2) + threadIdx.x;
        vf4 G[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) G[u] = g4[q0 + u * 256];      // (cached: the step reads g next)
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
            for (int c = 0; c < 4; ++c) take(G[u][c]);
    } else if (vec) {
        const long qb = e0 >> 2, q1 = e1 >> 2;   // whole float4s below e1 (e0 is a multiple of 4)
        const float4 *g4 = (const float4 *)t.g;
        if (q1 > qb) {                           // (uniform: a tensor of fewer than 4 elements has no float4 to clamp to)
            float4 G[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) G[u] = g4[min(qb + u * 256 + threadIdx.x, q1 - 1)];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const float keep = qb + u * 256 + threadIdx.x < q1 ? 1.f : 0.f;    // masked after the load: 0 is finite
                take(keep != 0.f ? G[u].x : 0.f); take(keep != 0.f ? G[u].y : 0.f);
                take(keep != 0.f ? G[u].z : 0.f); take(keep != 0.f ? G[u].w : 0.f);
            }
        }
        // tail of the tensor (n % 4 elements) belongs to the last chunk; e1 > e0, so e1 - 1 is an element of the tensor
        const long e = (q1 << 2) + threadIdx.x;
        const float g = t.g[min(e, e1 - 1)];
        take(e < e1 ? g : 0.f);
    } else {
        float G[ADAM_CHUNK / 256];
#pragma unroll
        for (int u = 0; u < ADAM_CHUNK / 256; ++u) G[u] = t.g[min(e0 + u * 256 + threadIdx.x, e1 - 1)];
#pragma unroll
        for (int u = 0; u < ADAM_CHUNK / 256; ++u) take(e0 + u * 256 + threadIdx.x < e1 ? G[u] : 0.f);
    }
    __shared__ double s_sum[4];
    __shared__ int s_bad[4];
    acc = wave_sum(acc);
    const bool wave_bad = __builtin_amdgcn_ballot_w64(bad) != 0;
    if ((threadIdx.x & 63) == 0) { s_sum[threadIdx.x >> 6] = acc; s_bad[threadIdx.x >> 6] = wave_bad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        CheckRow r;
        r.sumsq = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
        r.nonfinite = (s_bad[0] | s_bad[1] | s_bad[2] | s_bad[3]) ? 1.f : 0.f;
        r.reserved = 0.f;
        partial[blockIdx.x] = r;
    }
}

// the coefficients a finish kernel left in the optimizer's state
__device__ __forceinline__ AdamCoef state_coef(const ir2rgb_adam_state *__restrict__ st) {
    AdamCoef k;
    k.step_size = st->step_size; k.beta1 = st->beta1; k.beta2 = st->beta2; k.omb1 = st->omb1; k.omb2 = st->omb2;
    k.bc2_sqrt = st->bc2_sqrt; k.eps = st->eps;
    return k;
}

static inline bool misaligned(const void *p, unsigned a) { return ((uintptr_t)p & (a - 1)) != 0; }
