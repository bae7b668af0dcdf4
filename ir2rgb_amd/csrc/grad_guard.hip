// grad_guard.hip -- guarded optimizer steps for every compute dtype, decided on the device (gfx950): a gradient that holds
// an inf or a NaN skips its optimizer's step, a finite one is clipped to a global L2 norm.
//
// The same three launches as the loss-scaled step (loss_scale.hip), with one more rule in the middle one:
//     grad_check_kernel         (grad_check.h, shared) one read of g: finite? sum of squares, one row per workgroup
//     grad_guard_finish_kernel  found_inf, the unscaled norm, the clip coefficient and the factor the step multiplies g by;
//                               if finite, the step count and its coefficients -- ir2rgb_adam_state as ir2rgb_grad_check
//                               leaves it, plus the ir2rgb_grad_guard_state of this optimizer
//     adam_guarded_kernel       adam_kernel on g * factor, or nothing at all when found_inf is set
// With g the stored gradient (of the scaled loss when there is a loss scaler) and inv the scaler's inv_scale, or exactly 1
// without one, all in double:
//     norm = sqrt(sum g^2) * inv        c = min(1, max_norm / (norm + 1e-6))        factor = (float)(inv * c)
// which is torch.nn.utils.clip_grad_norm_ after the unscaling, except that torch evaluates c in fp32.  max_norm = +inf
// gives c = 1 exactly: factor is inv_scale (the loss-scaled step bit for bit) or 1.0 (the plain step bit for bit).
// Neither kernel uses LDS beyond the wave-sum rows, and neither uses scratch.
#include "grad_check.h"

static_assert(sizeof(ir2rgb_grad_guard_state) == 32, "ir2rgb_grad_guard_state layout");
static_assert(offsetof(ir2rgb_grad_guard_state, grad_norm) == 0 && offsetof(ir2rgb_grad_guard_state, clip_coef) == 4 &&
              offsetof(ir2rgb_grad_guard_state, factor) == 8 && offsetof(ir2rgb_grad_guard_state, steps) == 12 &&
              offsetof(ir2rgb_grad_guard_state, clipped) == 16 && offsetof(ir2rgb_grad_guard_state, skipped) == 20,
              "ir2rgb_grad_guard_state layout");

__global__ void __launch_bounds__(CHECK_FINISH_THREADS)
grad_guard_finish_kernel(const CheckRow *__restrict__ partial, int nrows, ir2rgb_adam_state *__restrict__ st,
                         ir2rgb_grad_guard_state *__restrict__ gs, const ir2rgb_loss_scale_state *__restrict__ sc,
                         float max_norm, float lr, float beta1, float beta2, float eps) {
    // the row sum of grad_check_finish_kernel (loss_scale.hip), in its order
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
        // ir2rgb_adam_state as grad_check_finish_kernel leaves it
        st->found_inf = found ? 1.f : 0.f;
        st->grad_sumsq = sumsq * (inv * inv);
        const double norm = sqrt(sumsq) * inv;
        gs->grad_norm = (float)norm;                               // (inf or NaN after a non-finite gradient)
        if (found) {
            gs->clip_coef = 0.f;
            gs->factor = 0.f;                                      // (not read: the step returns on found_inf)
            gs->skipped = gs->skipped + 1;
        } else {
            const int step = st->step + 1;
            const AdamCoef k = adam_coef(lr, beta1, beta2, eps, step);
            st->step = step;
            st->step_size = k.step_size; st->beta1 = k.beta1; st->beta2 = k.beta2; st->omb1 = k.omb1; st->omb2 = k.omb2;
            st->bc2_sqrt = k.bc2_sqrt; st->eps = k.eps;
            const double q = (double)max_norm / (norm + 1e-6);
            const double c = q < 1.0 ? q : 1.0;
            gs->clip_coef = (float)c;
            gs->factor = (float)(inv * c);
            gs->steps = gs->steps + 1;
            if (c < 1.0) gs->clipped = gs->clipped + 1;
        }
    }
}

__global__ void __launch_bounds__(256)
adam_guarded_kernel(const AdamTensor *__restrict__ table, const int2 *__restrict__ blocks,
                    const ir2rgb_adam_state *__restrict__ st, const ir2rgb_grad_guard_state *__restrict__ gs) {
    if (st->found_inf != 0.f) return;        // (uniform) the step is skipped: p, m, v stay as they are
    adam_block<true>(table, blocks, state_coef(st), gs->factor);
}

extern "C" long ir2rgb_grad_guard_state_bytes(void) { return (long)sizeof(ir2rgb_grad_guard_state); }

extern "C" int ir2rgb_grad_guard_check(const void *table, const void *blocks, int nblocks, void *partial, void *opt_state,
                                       void *guard_state, const void *scaler_state, float max_norm, float lr, float beta1,
                                       float beta2, float eps, void *stream) {
    if (!table || !blocks || !partial || !opt_state || !guard_state || nblocks < 0 || !(max_norm > 0.f) ||
        !(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f))
        return IR2RGB_EINVAL;
    if (misaligned(partial, 8) || misaligned(opt_state, 8) || misaligned(guard_state, 4) || misaligned(scaler_state, 4))
        return IR2RGB_EALIGN;
    if (nblocks > 0)
        grad_check_kernel<<<nblocks, 256, 0, as_stream(stream)>>>((const AdamTensor *)table, (const int2 *)blocks,
                                                                  (CheckRow *)partial);
    grad_guard_finish_kernel<<<1, CHECK_FINISH_THREADS, 0, as_stream(stream)>>>(
        (const CheckRow *)partial, nblocks, (ir2rgb_adam_state *)opt_state, (ir2rgb_grad_guard_state *)guard_state,
        (const ir2rgb_loss_scale_state *)scaler_state, max_norm, lr, beta1, beta2, eps);
    return ir2rgb_launch_status();
}

extern "C" int ir2rgb_adam_step_guarded(const void *table, const void *blocks, int nblocks, const void *opt_state,
                                        const void *guard_state, void *stream) {
    if (!table || !blocks || !opt_state || !guard_state || nblocks < 0) return IR2RGB_EINVAL;
    if (misaligned(opt_state, 8) || misaligned(guard_state, 4)) return IR2RGB_EALIGN;
    if (nblocks == 0) return IR2RGB_OK;
    adam_guarded_kernel<<<nblocks, 256, 0, as_stream(stream)>>>((const AdamTensor *)table, (const int2 *)blocks,
                                                                (const ir2rgb_adam_state *)opt_state,
                                                                (const ir2rgb_grad_guard_state *)guard_state);
    return ir2rgb_launch_status();
}
