// ema.hip -- exponential moving average of the generator's parameters as one streaming launch per window (gfx950,
// HBM-bound: 12 bytes per parameter: read p, read e, write e).
//
//     e <- e + alpha * (p - e),   alpha = 1 - beta_n
// over a device table of tensors {p, e, n}; `blocks` maps a workgroup to (tensor, chunk) as in adam.hip, with the same
// chunk size.  The three operations are rounded one by one (no contraction): p == e then leaves e as it is, bit for
// bit, so the average of a generator that is not being trained stays its parameters.  Nothing is selected: inf and NaN
// in p propagate as IEEE has them.
//
// The count of averages taken, the coefficient and the decision whether this window's average is taken at all live on
// the device (ir2rgb_ema_state; the generator optimizer's ir2rgb_adam_state for the decision):
//     ema_prepare_kernel   one thread: skip (found_inf) -> skipped += 1;  else updates += 1 and alpha of that update
//     ema_kernel           the stream; returns at once when found_inf is set, else reads alpha
// Both read found_inf from the same unchanged block, so they agree; the host reads nothing.
#include "adam.h"

static_assert(sizeof(ir2rgb_ema_state) == 16 && offsetof(ir2rgb_ema_state, updates) == 0 &&
              offsetof(ir2rgb_ema_state, skipped) == 4 && offsetof(ir2rgb_ema_state, alpha) == 8, "ir2rgb_ema_state layout");
static_assert(offsetof(ir2rgb_adam_state, found_inf) == 32, "ema_kernel reads found_inf of ir2rgb_adam_state");

struct EmaTensor {
    const float *p;
    float *e;
    long n;
};
static_assert(sizeof(EmaTensor) == 24, "the table row of ir2rgb_ema_step");

#define EMA_WARMUP_END (1 << 20)   // from here on beta_n = beta (and 1 + n, 10 + n below it are exact in fp32)

// One element: three roundings.  Contraction is off inside, as in adam_one (the _rn intrinsics are plain operators to
// hipcc and would be fused into e + alpha * d = fma(alpha, d, e) like any others).
__device__ __forceinline__ float ema_one(float p, float e, float alpha) {
#pragma clang fp contract(off)
    const float d = p - e;
    const float t = alpha * d;
    return e + t;
}

__global__ void __launch_bounds__(64)
ema_prepare_kernel(ir2rgb_ema_state *__restrict__ st, const ir2rgb_adam_state *__restrict__ opt, float beta, int warmup) {
    if (threadIdx.x != 0) return;
    if (opt != nullptr && opt->found_inf != 0.f) {      // the generator's step was skipped: so is its average
        st->skipped = st->skipped + 1;
        return;
    }
    const int n = st->updates + 1;
    float bn = beta;
    if (warmup && n < EMA_WARMUP_END) bn = fminf(beta, __fdiv_rn((float)(1 + n), (float)(10 + n)));
    st->updates = n;
    st->alpha = __fsub_rn(1.f, bn);
}

__global__ void __launch_bounds__(256)
ema_kernel(const EmaTensor *__restrict__ table, const int2 *__restrict__ blocks, const ir2rgb_ema_state *__restrict__ st,
           const ir2rgb_adam_state *__restrict__ opt) {
    if (opt != nullptr && opt->found_inf != 0.f) return;        // (uniform) skipped: e stays as it is
    const float alpha = st->alpha;
    const int2 tb = blocks[blockIdx.x];
    const EmaTensor t = table[tb.x];
    const long e0 = (long)tb.y * ADAM_CHUNK;
    const long e1 = min(t.n, e0 + ADAM_CHUNK);
    const bool vec = ((((uintptr_t)t.p | (uintptr_t)t.e) & 15) == 0);
    if (vec && e1 - e0 == ADAM_CHUNK) {
        // a whole chunk: no per-load bounds, global (not flat) accesses.  e is read and written once per window and by
        // nobody else: it bypasses the caches both ways.  p was just written by the Adam step and the weight repack reads
        // it next: a plain load.
        typedef float vf4 __attribute__((ext_vector_type(4)));
        typedef __attribute__((address_space(1))) vf4 gf4;
        const gf4 *p4 = (const gf4 *)(uintptr_t)t.p;
        gf4 *a4 = (gf4 *)(uintptr_t)t.e;
        const long q0 = (e0 >> 2) + threadIdx.x;
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            vf4 P[4], A[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const long q = q0 + (half * 4 + u) * 256;
                P[u] = p4[q];
                A[u] = __builtin_nontemporal_load(&a4[q]);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const long q = q0 + (half * 4 + u) * 256;
#pragma unroll
                for (int c = 0; c < 4; ++c) A[u][c] = ema_one(P[u][c], A[u][c], alpha);
                __builtin_nontemporal_store(A[u], &a4[q]);
            }
        }
    } else if (vec) {
        const long q1 = e1 >> 2;   // whole float4s below e1 (e0 is a multiple of 4)
        const float4 *p4 = (const float4 *)t.p;
        float4 *a4 = (float4 *)t.e;
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            float4 P[4], A[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const long q = (e0 >> 2) + (half * 4 + u) * 256 + threadIdx.x;
                if (q < q1) { P[u] = p4[q]; A[u] = a4[q]; }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const long q = (e0 >> 2) + (half * 4 + u) * 256 + threadIdx.x;
                if (q < q1) {
                    A[u].x = ema_one(P[u].x, A[u].x, alpha);
                    A[u].y = ema_one(P[u].y, A[u].y, alpha);
                    A[u].z = ema_one(P[u].z, A[u].z, alpha);
                    A[u].w = ema_one(P[u].w, A[u].w, alpha);
                    a4[q] = A[u];
                }
            }
        }
        // tail of the tensor (n % 4 elements) belongs to the last chunk
        for (long e = (q1 << 2) + threadIdx.x; e < e1; e += 256) t.e[e] = ema_one(t.p[e], t.e[e], alpha);
    } else {
        for (long e = e0 + threadIdx.x; e < e1; e += 256) t.e[e] = ema_one(t.p[e], t.e[e], alpha);
    }
}

extern "C" long ir2rgb_ema_state_bytes(void) { return (long)sizeof(ir2rgb_ema_state); }

extern "C" int ir2rgb_ema_step(const void *table, const void *blocks, int nblocks, void *ema_state, const void *opt_state,
                               float beta, int warmup, void *stream) {
    if (!table || !blocks || !ema_state || nblocks < 0 || !(beta >= 0.f && beta < 1.f)) return IR2RGB_EINVAL;
    if (misaligned(ema_state, 4) || misaligned(opt_state, 8)) return IR2RGB_EALIGN;
    if (nblocks == 0) return IR2RGB_OK;
    ema_prepare_kernel<<<1, 64, 0, as_stream(stream)>>>((ir2rgb_ema_state *)ema_state, (const ir2rgb_adam_state *)opt_state,
                                                        beta, warmup != 0);
    ema_kernel<<<nblocks, 256, 0, as_stream(stream)>>>((const EmaTensor *)table, (const int2 *)blocks,
                                                       (const ir2rgb_ema_state *)ema_state,
                                                       (const ir2rgb_adam_state *)opt_state);
    return ir2rgb_launch_status();
}
