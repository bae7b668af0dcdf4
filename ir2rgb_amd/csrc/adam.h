// adam.h -- what the two step kernels of adam.hip (plain and checked) share, and the chunk size ema.hip walks by: the
// table row, the coefficients of one step, the update of one element and the three paths of one (tensor, chunk) workgroup.
#pragma once
#include "common.h"

#define ADAM_CHUNK 8192   // elements per workgroup: 256 lanes x 8 float4

struct AdamTensor {
    float *p;
    const float *g;
    float *m;
    float *v;
    long n;
};

struct AdamCoef {
    float step_size, beta1, beta2, omb1, omb2, bc2_sqrt, eps;   // omb = 1 - beta, rounded from double like torch's
};

// The coefficients of step `step` (1-based) from the floats the entry points receive; host and device evaluate the same
// expressions in double (ir2rgb_adam_step on the host, grad_check_finish_kernel on the device).
static __host__ __device__ inline AdamCoef adam_coef(float lr, float beta1, float beta2, float eps, int step) {
    const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
    AdamCoef k;
    k.step_size = (float)((double)lr / bc1);
    k.beta1 = beta1;
    k.beta2 = beta2;
    k.omb1 = (float)(1.0 - (double)beta1);
    k.omb2 = (float)(1.0 - (double)beta2);
    k.bc2_sqrt = (float)sqrt(bc2);
    k.eps = eps;
    return k;
}

#ifdef __HIPCC__
// One element.  Every product-sum is spelled out and contraction is off inside, so that the rounding does not hang on
// what the compiler happens to fuse around it: adam_kernel and adam_checked_kernel then run the same arithmetic by
// construction (with equal coefficients the checked step on g is the plain step on g * factor bit for bit).  The
// forms are the ones the compiler had chosen for adam_kernel before they were pinned: v = fma(g, omb2 g, beta2 v) and
// p = fma(-step_size, m / denom, p) everywhere; m = fma(omb1, g, beta1 m) on the two float4 paths (FUSED_M) and
// beta1 m + omb1 g with both products rounded on the element-wise ones.
template <bool FUSED_M>
__device__ __forceinline__ void adam_one(float &p, float g, float &m, float &v, const AdamCoef &k) {
#pragma clang fp contract(off)
    const float step_size = k.step_size, bc2_sqrt = k.bc2_sqrt, eps = k.eps;
    const float bm = k.beta1 * m, og = k.omb1 * g;
    m = FUSED_M ? __builtin_fmaf(k.omb1, g, bm) : bm + og;
    const float o2g = k.omb2 * g, bv = k.beta2 * v;
    v = __builtin_fmaf(g, o2g, bv);
    const float denom = sqrtf(v) / bc2_sqrt + eps;
    p = __builtin_fmaf(-step_size, m / denom, p);
}

// One workgroup of 256 lanes on its (tensor, chunk).  SCALED: the gradient enters as g * inv_scale (the checked step
// passes its factor, inv_scale times the clip coefficient); otherwise inv_scale is not read.
template <bool SCALED>
__device__ __forceinline__ void adam_block(const AdamTensor *__restrict__ table, const int2 *__restrict__ blocks,
                                           const AdamCoef &k, const float inv_scale) {
    const int2 tb = blocks[blockIdx.x];
    const AdamTensor t = table[tb.x];
    const long e0 = (long)tb.y * ADAM_CHUNK;
    const long e1 = min(t.n, e0 + ADAM_CHUNK);
    const bool vec = ((((uintptr_t)t.p | (uintptr_t)t.g | (uintptr_t)t.m | (uintptr_t)t.v) & 15) == 0);
    if (vec && e1 - e0 == ADAM_CHUNK) {
        // a whole chunk (all but the last one of a tensor): no per-load bounds, global (not flat) accesses, and the
        // streams that nobody reads again before the next step (the gradient in, the two moments out) bypass the caches
        typedef float vf4 __attribute__((ext_vector_type(4)));
        typedef __attribute__((address_space(1))) vf4 gf4;
        gf4 *p4 = (gf4 *)(uintptr_t)t.p, *m4 = (gf4 *)(uintptr_t)t.m, *v4 = (gf4 *)(uintptr_t)t.v;
        const gf4 *g4 = (const gf4 *)(uintptr_t)t.g;
        const long q0 = (e0 >> 2) + threadIdx.x;
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            vf4 P[4], G[4], M[4], V[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const long q = q0 + (half * 4 + u) * 256;
                P[u] = p4[q];
                G[u] = __builtin_nontemporal_load(&g4[q]);
                M[u] = m4[q];
                V[u] = v4[q];
            }
            if constexpr (SCALED) {
#pragma unroll
                for (int u = 0; u < 4; ++u) G[u] = G[u] * inv_scale;       // one rounded product, exact for a power of two
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const long q = q0 + (half * 4 + u) * 256;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    float pp = P[u][c], mm = M[u][c], vv = V[u][c];
                    adam_one<true>(pp, G[u][c], mm, vv, k);
                    P[u][c] = pp; M[u][c] = mm; V[u][c] = vv;
                }
                p4[q] = P[u];
                __builtin_nontemporal_store(M[u], &m4[q]);
                __builtin_nontemporal_store(V[u], &v4[q]);
            }
        }
    } else if (vec) {
        const long q1 = e1 >> 2;   // whole float4s below e1 (e0 is a multiple of 4)
        float4 *p4 = (float4 *)t.p, *m4 = (float4 *)t.m, *v4 = (float4 *)t.v;
        const float4 *g4 = (const float4 *)t.g;
        // all loads of the chunk first (8 float4 per array per lane would be 128 VGPRs: two halves of 4)
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            float4 P[4], G[4], M[4], V[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const long q = (e0 >> 2) + (half * 4 + u) * 256 + threadIdx.x;
                if (q < q1) { P[u] = p4[q]; G[u] = g4[q]; M[u] = m4[q]; V[u] = v4[q]; }
            }
            if constexpr (SCALED) {
#pragma unroll
                for (int u = 0; u < 4; ++u) { G[u].x *= inv_scale; G[u].y *= inv_scale; G[u].z *= inv_scale; G[u].w *= inv_scale; }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const long q = (e0 >> 2) + (half * 4 + u) * 256 + threadIdx.x;
                if (q < q1) {
                    adam_one<true>(P[u].x, G[u].x, M[u].x, V[u].x, k);
                    adam_one<true>(P[u].y, G[u].y, M[u].y, V[u].y, k);
                    adam_one<true>(P[u].z, G[u].z, M[u].z, V[u].z, k);
                    adam_one<true>(P[u].w, G[u].w, M[u].w, V[u].w, k);
                    p4[q] = P[u]; m4[q] = M[u]; v4[q] = V[u];
                }
            }
        }
        // tail of the tensor (n % 4 elements) belongs to the last chunk
        for (long e = (q1 << 2) + threadIdx.x; e < e1; e += 256) {
            float p = t.p[e], m = t.m[e], v = t.v[e], g = t.g[e];
            if constexpr (SCALED) g *= inv_scale;
            adam_one<false>(p, g, m, v, k);
            t.p[e] = p; t.m[e] = m; t.v[e] = v;
        }
    } else {
        for (long e = e0 + threadIdx.x; e < e1; e += 256) {
            float p = t.p[e], m = t.m[e], v = t.v[e], g = t.g[e];
            if constexpr (SCALED) g *= inv_scale;
            adam_one<false>(p, g, m, v, k);
            t.p[e] = p; t.m[e] = m; t.v[e] = v;
        }
    }
}
#endif
