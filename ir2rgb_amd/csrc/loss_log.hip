// loss_log.hip -- the per-window loss record of a training run, kept on the device (gfx950).
//
// The reference reads its losses with two .item() calls per window and one per term every print_freq windows
// (train_vid2vid.py:99-100, :119-127).  Here one launch per window copies the window's loss scalars -- zero-dimensional
// fp32 tensors at addresses that differ from window to window -- into a ring, and adds them to fp64 running sums; the
// host reads the record when it prints.  The addresses travel in the kernel's argument block: no table upload, no
// staging buffer, nothing for the host to wait for.
// Latency-shaped like loss_scale_update_kernel (DESIGN, "Small kernels are latency-shaped"): one workgroup of one wave,
// lane = slot, every load of a lane in flight before the first use, loads unconditional from clamped addresses and
// masked afterwards, plain vector loads and stores, nothing atomic.
#include "common.h"

static_assert(sizeof(ir2rgb_loss_log_state) == 8 * (2 * IR2RGB_LOSS_LOG_SLOTS + 2) &&
              offsetof(ir2rgb_loss_log_state, skipped) == 16 * IR2RGB_LOSS_LOG_SLOTS, "ir2rgb_loss_log_state layout");
static_assert(IR2RGB_LOSS_LOG_SLOTS <= IR2RGB_WAVE, "one lane per slot");
static_assert(offsetof(ir2rgb_adam_state, found_inf) == 32, "found_inf of ir2rgb_adam_state");

struct LossLogArgs {
    const float *src[IR2RGB_LOSS_LOG_SLOTS];
    const ir2rgb_adam_state *opt[IR2RGB_LOSS_LOG_OPTIMIZERS];
};

__global__ void __launch_bounds__(IR2RGB_WAVE)
loss_log_push_kernel(const LossLogArgs a, unsigned present, int n_opts, float *__restrict__ ring, int capacity,
                     ir2rgb_loss_log_state *__restrict__ st) {
    const int lane = threadIdx.x;
    const int slot = min(lane, IR2RGB_LOSS_LOG_SLOTS - 1);
    const bool mine = lane < IR2RGB_LOSS_LOG_SLOTS && ((present >> slot) & 1u);
    // an absent slot reads the state block instead (any valid address: the value is masked below)
    const float *src = mine ? a.src[slot] : (const float *)st;
    const float v = *src;
    const double sum = st->sum[slot];
    const long long n = st->n[slot];
    const long long count = st->count, skipped = st->skipped;
    float f[IR2RGB_LOSS_LOG_OPTIMIZERS];
#pragma unroll
    for (int i = 0; i < IR2RGB_LOSS_LOG_OPTIMIZERS; ++i) {
        const ir2rgb_adam_state *o = a.opt[i < n_opts ? i : 0];
        f[i] = n_opts > 0 ? o->found_inf : 0.f;          // (uniform condition: without a scaler opt[] holds nothing)
    }
    bool skip = false;
#pragma unroll
    for (int i = 0; i < IR2RGB_LOSS_LOG_OPTIMIZERS; ++i) skip |= i < n_opts && f[i] != 0.f;
    if (lane < IR2RGB_LOSS_LOG_SLOTS) {
        const long row = (long)(count % capacity);
        ring[row * IR2RGB_LOSS_LOG_SLOTS + lane] = mine ? v : IR2RGB_LOSS_LOG_ABSENT;
        if (mine && !skip) {
            st->sum[lane] = sum + (double)v;
            st->n[lane] = n + 1;
        }
    }
    if (lane == 0) {
        st->count = count + 1;
        if (skip) st->skipped = skipped + 1;
    }
}

extern "C" int ir2rgb_loss_log_push(const void *const *srcs, unsigned present, int count, float *ring, int capacity,
                                    void *state, const void *const *opt_states, int n_opts, void *stream) {
    if (!srcs || !ring || !state || count < 0 || count > IR2RGB_LOSS_LOG_SLOTS || capacity <= 0 || n_opts < 0 ||
        n_opts > IR2RGB_LOSS_LOG_OPTIMIZERS || (n_opts > 0 && !opt_states))
        return IR2RGB_EINVAL;
    if (count < IR2RGB_LOSS_LOG_SLOTS && (present >> count) != 0u) return IR2RGB_EINVAL;    // a slot past the sources
    LossLogArgs a{};
    for (int i = 0; i < count; ++i) {
        if (!((present >> i) & 1u)) continue;
        if (!srcs[i]) return IR2RGB_EINVAL;
        if ((uintptr_t)srcs[i] & 3) return IR2RGB_EALIGN;
        a.src[i] = (const float *)srcs[i];
    }
    for (int i = 0; i < n_opts; ++i) {
        if (!opt_states[i]) return IR2RGB_EINVAL;
        if ((uintptr_t)opt_states[i] & 7) return IR2RGB_EALIGN;
        a.opt[i] = (const ir2rgb_adam_state *)opt_states[i];
    }
    if (((uintptr_t)ring & 3) || ((uintptr_t)state & 7)) return IR2RGB_EALIGN;
    loss_log_push_kernel<<<1, IR2RGB_WAVE, 0, as_stream(stream)>>>(a, present, n_opts, ring, capacity,
                                                                   (ir2rgb_loss_log_state *)state);
    return ir2rgb_launch_status();
}
