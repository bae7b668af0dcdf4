// adam.hip -- the optimizer step of the loop body (gfx950, HBM-bound: 28 bytes per parameter: read p, g, m, v,
// write p, m, v), plain as one launch per optimizer, or checked -- decided on the device -- as three.
//
// torch.optim.Adam(lr, betas, eps=1e-8, weight_decay=0, amsgrad=False) as the reference runs it
// (models/base_model.py / generator.py optimizer_G, discriminator.py optimizer_D; train_vid2vid.py:93-105):
//     m = beta1*m + (1-beta1)*g;  v = beta2*v + (1-beta2)*g*g
//     p = p - (lr / (1-beta1^t)) * m / (sqrt(v)/sqrt(1-beta2^t) + eps)
// over a device table of tensors {p, g, m, v, n}; `blocks` maps a workgroup to (tensor, chunk).
//
// The checked step serves f16 training's loss scale (an f16 activation gradient below 6e-5 loses bits and one below
// 6e-8 is gone, so the loss is multiplied by a scale before backward(): the reference's --fp16, apex's dynamic loss
// scaling; loss_scale.hip moves the scale) and the gradient guard of every compute dtype: a gradient that holds an inf
// or a NaN skips its optimizer's step, a finite one is unscaled and clipped to a global L2 norm.  The host never reads
// the decision:
//     grad_check_kernel         one read of g (4 B per parameter on top of the step's 28): finite? sum of squares, one
//                               row per (tensor, chunk) workgroup
//     grad_check_finish_kernel  one workgroup sums the rows in row order and applies the rule: found_inf, the unscaled
//                               norm, the factor the step multiplies g by and -- if finite -- the step count and its
//                               coefficients, in ir2rgb_adam_state; the guard's figures and counters when there is one
//     adam_checked_kernel       adam_kernel on g * factor, or nothing at all when found_inf is set
// With g the stored gradient (of the scaled loss when there is a loss scaler) and inv the scaler's inv_scale, or exactly 1
// without one, all in double:
//     norm = sqrt(sum g^2) * inv        c = min(1, max_norm / (norm + 1e-6))        factor = (float)(inv * c)
// which is torch.nn.utils.clip_grad_norm_ after the unscaling, except that torch evaluates c in fp32.  max_norm = +inf
// gives c = 1 exactly: factor is inv_scale bit for bit, or 1.0 (the plain step bit for bit).
// The check and the finish are latency-shaped (DESIGN, "Small kernels are latency-shaped"): every load of a thread is
// in flight before the first use, loads are unconditional from clamped indices and masked afterwards, sums are in
// double in a fixed order (thread, wave, workgroup, row), and nothing is atomic.  Neither uses LDS beyond the wave-sum
// rows, and no kernel here uses scratch.
#include "adam.h"

static_assert(sizeof(ir2rgb_adam_state) == 48 && offsetof(ir2rgb_adam_state, factor) == 36 &&
              offsetof(ir2rgb_adam_state, grad_sumsq) == 40, "ir2rgb_adam_state layout");
static_assert(offsetof(ir2rgb_adam_state, step_size) == 4 && offsetof(ir2rgb_adam_state, found_inf) == 32 &&
              sizeof(AdamCoef) == 28, "the coefficients of ir2rgb_adam_state are an AdamCoef");
static_assert(sizeof(ir2rgb_grad_guard_state) == 32, "ir2rgb_grad_guard_state layout");
static_assert(offsetof(ir2rgb_grad_guard_state, grad_norm) == 0 && offsetof(ir2rgb_grad_guard_state, clip_coef) == 4 &&
              offsetof(ir2rgb_grad_guard_state, factor) == 8 && offsetof(ir2rgb_grad_guard_state, steps) == 12 &&
              offsetof(ir2rgb_grad_guard_state, clipped) == 16 && offsetof(ir2rgb_grad_guard_state, skipped) == 20,
              "ir2rgb_grad_guard_state layout");

struct CheckRow {
    double sumsq;
    float nonfinite, reserved;
};
static_assert(sizeof(CheckRow) == 16, "one 16-byte load per partial row");

#define CHECK_FINISH_THREADS 1024

__global__ void __launch_bounds__(256)
adam_kernel(const AdamTensor *__restrict__ table, const int2 *__restrict__ blocks, const AdamCoef k) {
    adam_block<false>(table, blocks, k, 1.f);
}

__global__ void __launch_bounds__(256)
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

// gs NULL: no guard block is written.  sc NULL: inv is exactly 1.
__global__ void __launch_bounds__(CHECK_FINISH_THREADS)
grad_check_finish_kernel(const CheckRow *__restrict__ partial, int nrows, ir2rgb_adam_state *__restrict__ st,
                         ir2rgb_grad_guard_state *__restrict__ gs, const ir2rgb_loss_scale_state *__restrict__ sc,
                         float max_norm, float lr, float beta1, float beta2, float eps) {
    typedef unsigned uv4 __attribute__((ext_vector_type(4)));
    const uv4 *rows = (const uv4 *)partial;
    double acc = 0.0;
    bool bad = false;
    // eight rows per thread and trip, all in flight at once; row r of a trip is summed before row r + 1024
    for (int base = 0; base < nrows; base += 8 * CHECK_FINISH_THREADS) {
        uv4 R[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) R[u] = rows[min(base + u * CHECK_FINISH_THREADS + (int)threadIdx.x, nrows - 1)];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const bool in = base + u * CHECK_FINISH_THREADS + (int)threadIdx.x < nrows;
            const double s = __longlong_as_double(((long long)R[u].y << 32) | (long long)R[u].x);
            acc += in ? s : 0.0;
            bad |= in && __uint_as_float(R[u].z) != 0.f;
        }
    }
    __shared__ double s_sum[CHECK_FINISH_THREADS / 64];
    __shared__ int s_bad[CHECK_FINISH_THREADS / 64];
    acc = wave_sum(acc);
    const bool wave_bad = __builtin_amdgcn_ballot_w64(bad) != 0;
    if ((threadIdx.x & 63) == 0) { s_sum[threadIdx.x >> 6] = acc; s_bad[threadIdx.x >> 6] = wave_bad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double sumsq = 0.0;
        int found = 0;
#pragma unroll
        for (int w = 0; w < CHECK_FINISH_THREADS / 64; ++w) { sumsq += s_sum[w]; found |= s_bad[w]; }
        const double inv = sc ? (double)sc->inv_scale : 1.0;       // (uniform)
        const double norm = sqrt(sumsq) * inv;                     // (inf or NaN after a non-finite gradient)
        double c = 0.0;
        float factor = 0.f;                                        // (not read after found: the step returns on found_inf)
        st->found_inf = found ? 1.f : 0.f;
        st->grad_sumsq = sumsq * (inv * inv);
        if (!found) {
            const int step = st->step + 1;
            const AdamCoef k = adam_coef(lr, beta1, beta2, eps, step);
            st->step = step;
            st->step_size = k.step_size; st->beta1 = k.beta1; st->beta2 = k.beta2; st->omb1 = k.omb1; st->omb2 = k.omb2;
            st->bc2_sqrt = k.bc2_sqrt; st->eps = k.eps;
            const double q = (double)max_norm / (norm + 1e-6);
            c = q < 1.0 ? q : 1.0;
            factor = (float)(inv * c);
        }
        st->factor = factor;
        if (gs) {
            gs->grad_norm = (float)norm;
            gs->clip_coef = (float)c;
            gs->factor = factor;
            if (found) {
                gs->skipped = gs->skipped + 1;
            } else {
                gs->steps = gs->steps + 1;
                if (c < 1.0) gs->clipped = gs->clipped + 1;
            }
        }
    }
}

__global__ void __launch_bounds__(256)
adam_checked_kernel(const AdamTensor *__restrict__ table, const int2 *__restrict__ blocks,
                    const ir2rgb_adam_state *__restrict__ st) {
    if (st->found_inf != 0.f) return;        // (uniform) the step is skipped: p, m, v stay as they are
    AdamCoef k;                              // the coefficients the finish kernel left
    k.step_size = st->step_size; k.beta1 = st->beta1; k.beta2 = st->beta2; k.omb1 = st->omb1; k.omb2 = st->omb2;
    k.bc2_sqrt = st->bc2_sqrt; k.eps = st->eps;
    adam_block<true>(table, blocks, k, st->factor);
}

extern "C" int ir2rgb_adam_chunk_elems(void) { return ADAM_CHUNK; }

extern "C" long ir2rgb_grad_check_partial_bytes(int nblocks) {
    if (nblocks < 0) return IR2RGB_EINVAL;
    return (long)sizeof(CheckRow) * (nblocks > 0 ? nblocks : 1);
}

extern "C" long ir2rgb_grad_guard_state_bytes(void) { return (long)sizeof(ir2rgb_grad_guard_state); }

extern "C" int ir2rgb_adam_step(const void *table, const void *blocks, int nblocks, float lr, float beta1, float beta2,
                                float eps, int step, void *stream) {
    if (!table || !blocks || nblocks < 0 || step < 1 || !(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f))
        return IR2RGB_EINVAL;
    if (nblocks == 0) return IR2RGB_OK;
    const AdamCoef k = adam_coef(lr, beta1, beta2, eps, step);
    adam_kernel<<<nblocks, 256, 0, as_stream(stream)>>>((const AdamTensor *)table, (const int2 *)blocks, k);
    return ir2rgb_launch_status();
}

extern "C" int ir2rgb_grad_check(const void *table, const void *blocks, int nblocks, void *partial, void *opt_state,
                                 void *guard_state, const void *scaler_state, float max_norm, float lr, float beta1,
                                 float beta2, float eps, void *stream) {
    if (!table || !blocks || !partial || !opt_state || nblocks < 0 || !(max_norm > 0.f) ||
        !(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f))
        return IR2RGB_EINVAL;
    if (misaligned(partial, 8) || misaligned(opt_state, 8) || misaligned(guard_state, 4) || misaligned(scaler_state, 4))
        return IR2RGB_EALIGN;
    if (nblocks > 0)
        grad_check_kernel<<<nblocks, 256, 0, as_stream(stream)>>>((const AdamTensor *)table, (const int2 *)blocks,
                                                                  (CheckRow *)partial);
    grad_check_finish_kernel<<<1, CHECK_FINISH_THREADS, 0, as_stream(stream)>>>(
        (const CheckRow *)partial, nblocks, (ir2rgb_adam_state *)opt_state, (ir2rgb_grad_guard_state *)guard_state,
        (const ir2rgb_loss_scale_state *)scaler_state, max_norm, lr, beta1, beta2, eps);
    return ir2rgb_launch_status();
}

extern "C" int ir2rgb_adam_step_checked(const void *table, const void *blocks, int nblocks, const void *opt_state,
                                        void *stream) {
    if (!table || !blocks || !opt_state || nblocks < 0) return IR2RGB_EINVAL;
    if (misaligned(opt_state, 8)) return IR2RGB_EALIGN;
    if (nblocks == 0) return IR2RGB_OK;
    adam_checked_kernel<<<nblocks, 256, 0, as_stream(stream)>>>((const AdamTensor *)table, (const int2 *)blocks,
                                                                (const ir2rgb_adam_state *)opt_state);
    return ir2rgb_launch_status();
}
