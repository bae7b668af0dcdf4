// adam.hip -- the optimizer step of the loop body as one launch per optimizer (gfx950, HBM-bound:
// 28 bytes per parameter: read p, g, m, v, write p, m, v).
//
// torch.optim.Adam(lr, betas, eps=1e-8, weight_decay=0, amsgrad=False) as the reference runs it
// (models/base_model.py / generator.py optimizer_G, discriminator.py optimizer_D; train_vid2vid.py:93-105):
//     m = beta1*m + (1-beta1)*g;  v = beta2*v + (1-beta2)*g*g
//     p = p - (lr / (1-beta1^t)) * m / (sqrt(v)/sqrt(1-beta2^t) + eps)
// over a device table of tensors {p, g, m, v, n}; `blocks` maps a workgroup to (tensor, chunk).
#include "adam.h"

__global__ void __launch_bounds__(256)
adam_kernel(const AdamTensor *__restrict__ table, const int2 *__restrict__ blocks, const AdamCoef k) {
    adam_block<false>(table, blocks, k, 1.f);
}

extern "C" int ir2rgb_adam_chunk_elems(void) { return ADAM_CHUNK; }

extern "C" int ir2rgb_adam_step(const void *table, const void *blocks, int nblocks, float lr, float beta1, float beta2,
                                float eps, int step, void *stream) {
    if (!table || !blocks || nblocks < 0 || step < 1 || !(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f))
        return IR2RGB_EINVAL;
    if (nblocks == 0) return IR2RGB_OK;
    const AdamCoef k = adam_coef(lr, beta1, beta2, eps, step);
    adam_kernel<<<nblocks, 256, 0, as_stream(stream)>>>((const AdamTensor *)table, (const int2 *)blocks, k);
    return ir2rgb_launch_status();
}
