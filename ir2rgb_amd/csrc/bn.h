// bn.h -- the BatchNorm formulas that pointwise.hip (forward) and backward.hip share.  A fused kernel that promises results
// bit-identical to the launches it replaces calls the same function here; it does not keep a copy in step by hand.
// (Written out in the kernels for measured reasons: the forward 8-channel apply, and all of bn_bwd_onepass_kernel.)
#pragma once
#include "common.h"

// Pixel chunks of a [npix][C] tensor for the kernels whose blocks own a 64-channel slice and a pixel range: about
// `blocks` workgroups in all (between lo and hi chunks per slice), at least 128 pixels per chunk.
struct BnChunks {
    long per;       // pixels per chunk
    int n;          // chunks that hold a pixel
};
static inline BnChunks bn_chunks(long npix, int C, long blocks, long lo, long hi) {
    long want = blocks / (C / 64);
    want = want < lo ? lo : (want > hi ? hi : want);
    const long cap = (npix + 127) / 128;
    want = want < cap ? want : cap;
    const long per = (npix + want - 1) / want;
    return {per, (int)((npix + per - 1) / per)};
}
// the apply half of the fused kernels (forward and backward): about 2048 blocks
static inline BnChunks bn_apply_chunks(long npix, int C) { return bn_chunks(npix, C, 2048, 1, npix); }

#ifdef __HIPCC__
// ---- forward ------------------------------------------------------------------------------------------------------
// Channel c from its two sums over `count` pixels (double): var = E[y^2] - E[y]^2, scale = gamma * invstd,
// shift = beta - mean * scale.  publish: also store the four vectors and update the running statistics.
//   stat_updates > 1: this forward stands for that many identical forwards of the reference.
//   conv_bias: the statistics are those of the bias-free convolution output; nn.BatchNorm2d saw y + bias
struct BnScaleShift {
    float sc, sh;
};
__device__ __forceinline__ BnScaleShift bn_channel_stats(double s1, double s2, double count, int c, const float *gamma,
                                                 const float *beta, const float *conv_bias, float *running_mean,
                                                 float *running_var, float momentum, float eps, int stat_updates,
                                                 bool publish, float *scale, float *shift, float *mean_out,
                                                 float *invstd_out) {
    const double mean = s1 / count;
    double var = s2 / count - mean * mean;
    var = (var > 0.0 || var != var) ? var : 0.0;      // (a NaN variance -- an overflowed forward -- stays NaN)
    const float invstd = (float)(1.0 / sqrt(var + (double)eps));
    const float g = gamma ? gamma[c] : 1.f, b = beta ? beta[c] : 0.f;
    const float sc = g * invstd, sh = b - (float)mean * sc;
    if (!publish) return {sc, sh};
    scale[c] = sc;
    shift[c] = sh;
    if (mean_out) mean_out[c] = (float)mean;
    if (invstd_out) invstd_out[c] = invstd;
    if (running_mean) {
        float r = running_mean[c];
        const float m = (float)mean + (conv_bias ? conv_bias[c] : 0.f);
        for (int u = 0; u < stat_updates; ++u) r = (1.f - momentum) * r + momentum * m;
        running_mean[c] = r;
    }
    if (running_var) {
        const double unbiased = count > 1.0 ? var * count / (count - 1.0) : var;
        float r = running_var[c];
        for (int u = 0; u < stat_updates; ++u) r = (1.f - momentum) * r + momentum * (float)unbiased;
        running_var[c] = r;
    }
    return {sc, sh};
}

// ---- backward -----------------------------------------------------------------------------------------------------
// s1 += g', s2 += g' * yhat on the 8 channels of a lane: g' = gz * act'(y*scale + shift), yhat = (y - mean) * invstd
// (ok = false: a masked row adds nothing)
__device__ __forceinline__ void bn_bwd_sums8(uint4 gq, uint4 yq, const float *sc, const float *sh,
                                             const float *mu, const float *is, int act, int dt, bool ok, float *s1,
                                             float *s2) {
    float g[8], v[8];
    unpack8(gq, g, dt);
    unpack8(yq, v, dt);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float gp = ok ? act_grad(g[j], v[j] * sc[j] + sh[j], act) : 0.f;
        s1[j] += gp;
        s2[j] += gp * (v[j] - mu[j]) * is[j];
    }
}

// Rows k, k + 8, ..., k + 120 (those below R) of one column of the [R][2][C] partial sums, in double.  The 16 loads
// are unconditional on a clamped row and masked afterwards: a predicated load compiles to a branch with its own
// s_waitcnt (16 serial round trips).
__device__ __forceinline__ double bn_bwd_slice_sum(const float *__restrict__ partial, int k, int R, int which, int C,
                                                   int c) {
    float t[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) t[u] = partial[((long)min(k + 8 * u, R - 1) * 2 + which) * C + c];
    double a = 0.0;
#pragma unroll
    for (int u = 0; u < 16; ++u) a += k + 8 * u < R ? (double)t[u] : 0.0;
    return a;
}

// Channel c from its two sums a = sum g', b = sum g' * yhat: the parameter gradients (acc: those of an earlier sample
// group of the same layer are already there) ...
__device__ __forceinline__ void bn_bwd_param_grads(double a, double b, int c, float *dgamma, float *dbeta, int acc) {
    dbeta[c] = (acc ? dbeta[c] : 0.f) + (float)a;
    dgamma[c] = (acc ? dgamma[c] : 0.f) + (float)b;
}
// ... and the three coefficients of gy = cA*g' + cB*y + cC:
//   cA = scale, cB = -scale*invstd*dgamma/n, cC = scale*(invstd*mean*dgamma/n - dbeta/n)   (inv_n = 0: frozen statistics)
__device__ __forceinline__ void bn_bwd_coef(double a, double b, float scv, float isv, float muv, float inv_n, float &cA,
                                            float &cB, float &cC) {
    const float dg = (float)b * inv_n, db = (float)a * inv_n;
    cA = scv;
    cB = -scv * isv * dg;
    cC = scv * (isv * muv * dg - db);
}
// The contraction is written out: left to hipcc, which product joins the fma changes with the code around the call (packed
// or scalar, inlined where) and the low bit of gy with it.  fma(cB, y, cA*g') is what the fused kernel has always computed.
__device__ __forceinline__ uint4 bn_bwd_gy8(uint4 gq, uint4 yq, const float *sc, const float *sh, const float *cA,
                                            const float *cB, const float *cC, int act, int dt) {
    float g[8], v[8], o[8];
    unpack8(gq, g, dt);
    unpack8(yq, v, dt);
#pragma unroll
    for (int j = 0; j < 8; ++j)
        o[j] = __builtin_fmaf(cB[j], v[j], cA[j] * act_grad(g[j], v[j] * sc[j] + sh[j], act)) + cC[j];
    return pack8(o, dt);
}
#endif
