// loss_scale.hip -- dynamic loss scaling for f16 training, decided on the device (gfx950).
//
// An f16 activation gradient below 6e-5 loses bits and one below 6e-8 is gone, so the loss is multiplied by a scale
// before backward() (the reference's --fp16, apex's dynamic loss scaling).  What follows the backward pass stays on
// the device -- the host never reads the decision:
//     grad_check_kernel         (grad_check.h, shared with grad_guard.hip) one read of g (4 B per parameter on top of
//                               the step's 28): finite? sum of squares
//     grad_check_finish_kernel  found_inf, the unscaled norm, and -- if finite -- the step count and its coefficients
//     adam_scaled_kernel        adam_kernel on g * inv_scale, or nothing at all when found_inf is set
//     loss_scale_update_kernel  torch._amp_update_scale_'s rule over the optimizers stepped this window
// The check and the update are latency-shaped (DESIGN, "Small kernels are latency-shaped"): every load of a thread is
// in flight before the first use, loads are unconditional from clamped indices and masked afterwards, sums are in
// double in a fixed order (thread, wave, workgroup), and nothing is atomic.
#include "grad_check.h"

static_assert(sizeof(ir2rgb_adam_state) == 48 && offsetof(ir2rgb_adam_state, grad_sumsq) == 40, "ir2rgb_adam_state layout");
static_assert(offsetof(ir2rgb_adam_state, step_size) == 4 && offsetof(ir2rgb_adam_state, found_inf) == 32 &&
              sizeof(AdamCoef) == 28, "the coefficients of ir2rgb_adam_state are an AdamCoef");
static_assert(sizeof(ir2rgb_loss_scale_state) == 16, "ir2rgb_loss_scale_state layout");

#define LOSS_SCALE_MAX_OPTIMIZERS 8

__global__ void __launch_bounds__(CHECK_FINISH_THREADS)
grad_check_finish_kernel(const CheckRow *__restrict__ partial, int nrows, ir2rgb_adam_state *__restrict__ st,
                         const ir2rgb_loss_scale_state *__restrict__ sc, float lr, float beta1, float beta2, float eps) {
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
        const double inv = (double)sc->inv_scale;
        st->found_inf = found ? 1.f : 0.f;
        st->grad_sumsq = sumsq * (inv * inv);
        if (!found) {
            const int step = st->step + 1;
            const AdamCoef k = adam_coef(lr, beta1, beta2, eps, step);
            st->step = step;
            st->step_size = k.step_size; st->beta1 = k.beta1; st->beta2 = k.beta2; st->omb1 = k.omb1; st->omb2 = k.omb2;
            st->bc2_sqrt = k.bc2_sqrt; st->eps = k.eps;
        }
    }
}

__global__ void __launch_bounds__(256)
adam_scaled_kernel(const AdamTensor *__restrict__ table, const int2 *__restrict__ blocks,
                   const ir2rgb_adam_state *__restrict__ st, const ir2rgb_loss_scale_state *__restrict__ sc) {
    if (st->found_inf != 0.f) return;        // (uniform) the step is skipped: p, m, v stay as they are
    adam_block<true>(table, blocks, state_coef(st), sc->inv_scale);
}

__global__ void __launch_bounds__(64)
loss_scale_update_kernel(ir2rgb_loss_scale_state *__restrict__ sc, const ir2rgb_adam_state *const *__restrict__ opts,
                         int count, float growth, float backoff, int growth_interval) {
    if (threadIdx.x != 0) return;
    // all flags in flight at once: addresses from a clamped index, then the flags, masked afterwards
    const ir2rgb_adam_state *o[LOSS_SCALE_MAX_OPTIMIZERS];
    float f[LOSS_SCALE_MAX_OPTIMIZERS];
#pragma unroll
    for (int i = 0; i < LOSS_SCALE_MAX_OPTIMIZERS; ++i) o[i] = opts[min(i, count - 1)];
#pragma unroll
    for (int i = 0; i < LOSS_SCALE_MAX_OPTIMIZERS; ++i) f[i] = o[i]->found_inf;
    bool found = false;
#pragma unroll
    for (int i = 0; i < LOSS_SCALE_MAX_OPTIMIZERS; ++i) found |= i < count && f[i] != 0.f;
    float scale = sc->scale;
    int tracker = sc->growth_tracker;
    if (found) sc->skipped = sc->skipped + 1;
    if (growth_interval == 0) return;        // a static scale: steps are skipped, the scale stays
    if (found) {
        scale = (float)((double)scale * (double)backoff);
        tracker = 0;
    } else if (++tracker == growth_interval) {
        const float grown = (float)((double)scale * (double)growth);
        if (!nonfinite(grown)) scale = grown;
        tracker = 0;
    }
    sc->scale = scale;
    sc->inv_scale = (float)(1.0 / (double)scale);
    sc->growth_tracker = tracker;
}

extern "C" long ir2rgb_loss_scale_state_bytes(int which) {
    if (which == 0) return (long)sizeof(ir2rgb_adam_state);
    if (which == 1) return (long)sizeof(ir2rgb_loss_scale_state);
    return IR2RGB_EINVAL;
}

extern "C" long ir2rgb_grad_check_partial_bytes(int nblocks) {
    if (nblocks < 0) return IR2RGB_EINVAL;
    return (long)sizeof(CheckRow) * (nblocks > 0 ? nblocks : 1);
}

extern "C" int ir2rgb_grad_check(const void *table, const void *blocks, int nblocks, void *partial, void *opt_state,
                                 const void *scaler_state, float lr, float beta1, float beta2, float eps, void *stream) {
    if (!table || !blocks || !partial || !opt_state || !scaler_state || nblocks < 0 || !(beta1 >= 0.f && beta1 < 1.f) ||
        !(beta2 >= 0.f && beta2 < 1.f))
        return IR2RGB_EINVAL;
    if (misaligned(partial, 8) || misaligned(opt_state, 8) || misaligned(scaler_state, 4)) return IR2RGB_EALIGN;
    if (nblocks > 0)
        grad_check_kernel<<<nblocks, 256, 0, as_stream(stream)>>>((const AdamTensor *)table, (const int2 *)blocks,
                                                                  (CheckRow *)partial);
    grad_check_finish_kernel<<<1, CHECK_FINISH_THREADS, 0, as_stream(stream)>>>(
        (const CheckRow *)partial, nblocks, (ir2rgb_adam_state *)opt_state, (const ir2rgb_loss_scale_state *)scaler_state,
        lr, beta1, beta2, eps);
    return ir2rgb_launch_status();
}

extern "C" int ir2rgb_adam_step_scaled(const void *table, const void *blocks, int nblocks, const void *opt_state,
                                       const void *scaler_state, void *stream) {
    if (!table || !blocks || !opt_state || !scaler_state || nblocks < 0) return IR2RGB_EINVAL;
    if (misaligned(opt_state, 8) || misaligned(scaler_state, 4)) return IR2RGB_EALIGN;
    if (nblocks == 0) return IR2RGB_OK;
    adam_scaled_kernel<<<nblocks, 256, 0, as_stream(stream)>>>((const AdamTensor *)table, (const int2 *)blocks,
                                                               (const ir2rgb_adam_state *)opt_state,
                                                               (const ir2rgb_loss_scale_state *)scaler_state);
    return ir2rgb_launch_status();
}

extern "C" int ir2rgb_loss_scale_update(void *scaler_state, const void *opt_states, int count, float growth, float backoff,
                                        int growth_interval, void *stream) {
    if (!scaler_state || !opt_states || count < 0 || count > LOSS_SCALE_MAX_OPTIMIZERS || growth_interval < 0 ||
        !(growth >= 1.f) || !(backoff > 0.f && backoff <= 1.f))
        return IR2RGB_EINVAL;
    if (misaligned(scaler_state, 4) || misaligned(opt_states, 8)) return IR2RGB_EALIGN;
    if (count == 0) return IR2RGB_OK;
    loss_scale_update_kernel<<<1, 64, 0, as_stream(stream)>>>((ir2rgb_loss_scale_state *)scaler_state,
                                                              (const ir2rgb_adam_state *const *)opt_states, count, growth,
                                                              backoff, growth_interval);
    return ir2rgb_launch_status();
}
