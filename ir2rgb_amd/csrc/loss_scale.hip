// loss_scale.hip -- the scale of f16 training's dynamic loss scaling, moved on the device (gfx950).
//
// The loss is multiplied by the scale before backward(); the checked step of adam.hip unscales, checks and steps or
// skips, and leaves its decision in every optimizer's ir2rgb_adam_state.  Once per window
//     loss_scale_update_kernel  torch._amp_update_scale_'s rule over the optimizers stepped this window
// reads those decisions -- the host never does.  It is latency-shaped (DESIGN, "Small kernels are latency-shaped"): one
// thread, every load in flight before the first use, unconditional from clamped indices and masked afterwards.
#include "common.h"

static_assert(sizeof(ir2rgb_adam_state) == 48 && offsetof(ir2rgb_adam_state, found_inf) == 32,
              "loss_scale_update_kernel reads found_inf of ir2rgb_adam_state");
static_assert(sizeof(ir2rgb_loss_scale_state) == 16, "ir2rgb_loss_scale_state layout");

#define LOSS_SCALE_MAX_OPTIMIZERS 8

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
