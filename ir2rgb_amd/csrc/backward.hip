// backward.hip -- HBM-bound backward companions of the MFMA convolution (gfx950):
//   * bn_bwd_onepass, or bn_bwd_reduce + bn_bwd_finalize_apply : backward of activation + BatchNorm2d on NHWC half
//     tensors, producing the gradient w.r.t. the convolution output plus dgamma / dbeta (formulas: bn.h);
//     bn_bwd_reduce + bn_bwd_finalize + bn_bwd_apply : the same for a norm-less stage (activation and bias gradient);
//   * fold_reflect : adjoint of nn.ReflectionPad2d -- folds the border of the padded-domain
//     gradient produced by the data-gradient convolution back into the image;
//   * xexpand_bwd  : adjoint of the x-direction im2col of the first layers.
// Reductions are two-level and deterministic (per-block partial rows, then a finalize kernel).
#include "bn.h"

// One block (512 threads) = one 64-channel group x one pixel range.  partial[r][0][c] = sum g',
// partial[r][1][c] = sum g' * yhat over range r.  Thread t owns channel octet t & 7 of the group
// and pixel rows (t >> 3) + 64k of the range, four rows in flight: a dependent HBM round trip
// costs ~2 us here, so these small reductions are shaped to need as few of them as possible.
// (A last-block-finalises variant was measured: the device-scope fences it needs write back the
// XCD L2s and made this kernel 4x slower than reduce + a separate finalize launch.  With 1024 threads the
// 128-VGPR cap made the compiler spill 18 registers: scratch costs dispatch latency, ~14 us floor per call.)
__global__ void __launch_bounds__(512)
bn_bwd_reduce_kernel(const uint4 *__restrict__ gz, const uint4 *__restrict__ y, const float *__restrict__ scale,
                     const float *__restrict__ shift, const float *__restrict__ mean, const float *__restrict__ invstd,
                     float *__restrict__ partial, long npix, int C, int act, int dt, long pix_per_block) {
    __shared__ float red[2][8][64];
    const int octs = C >> 3, ngroups = C >> 6;
    const int cg = blockIdx.x % ngroups, r = blockIdx.x / ngroups;
    const int oc = threadIdx.x & 7, row = threadIdx.x >> 3, wave = threadIdx.x >> 6;
    const long p_begin = (long)r * pix_per_block;
    const long p_end = min(npix, p_begin + pix_per_block);
    const int c0 = cg * 64 + oc * 8;
    float s1[8], s2[8], sc[8], sh[8], mu[8], is[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        s1[j] = s2[j] = 0.f;
        sc[j] = scale ? scale[c0 + j] : 1.f;
        sh[j] = shift ? shift[c0 + j] : 0.f;
        mu[j] = mean ? mean[c0 + j] : 0.f;
        is[j] = invstd ? invstd[c0 + j] : 1.f;
    }
    const long lane_off = (long)cg * 8 + oc;
    for (long p = p_begin + row; p < p_end; p += 256) {
        uint4 gq[4], yq[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long q = p + 64 * u;
            const bool ok = q < p_end;
            gq[u] = ok ? gz[q * octs + lane_off] : make_uint4(0, 0, 0, 0);
            yq[u] = ok ? y[q * octs + lane_off] : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) bn_bwd_sums8(gq[u], yq[u], sc, sh, mu, is, act, dt, true, s1, s2);   // g == 0 for the padding rows
    }
    // the 8 pixel rows of a wave (lane bits 3..5), then the 8 waves through LDS in wave order
#pragma unroll
    for (int j = 0; j < 8; ++j) {
#pragma unroll
        for (int m = 8; m < 64; m <<= 1) {
            s1[j] += __shfl_xor(s1[j], m);
            s2[j] += __shfl_xor(s2[j], m);
        }
    }
    if ((threadIdx.x & 63) < 8) {
#pragma unroll
        for (int j = 0; j < 8; ++j) { red[0][wave][oc * 8 + j] = s1[j]; red[1][wave][oc * 8 + j] = s2[j]; }
    }
    __syncthreads();
    if (threadIdx.x < 128) {
        const int which = threadIdx.x >> 6, cl = threadIdx.x & 63;
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) s += red[which][k][cl];
        partial[((long)r * 2 + which) * C + cg * 64 + cl] = s;
    }
}

// The two kernels behind bn_bwd_reduce_kernel for a stage WITHOUT a norm layer (scale == nullptr there: g' = gz * act'(y)).
// One block (1024 threads) per 64-channel group: dbeta[c] = sum_r partial[r][0][c], the bias gradient, and
// dgamma[c] = sum_r partial[r][1][c] (R <= 128 rows: thread = (value, slice of 16 rows), every load of a thread in
// flight at once; slices and rows are added in a fixed order, in double).
__global__ void __launch_bounds__(1024)
bn_bwd_finalize_kernel(const float *__restrict__ partial, int R, int C, float *__restrict__ dgamma,
                       float *__restrict__ dbeta, int acc) {
    __shared__ double fin[8][2][64];
    const int cg = blockIdx.x;
    {
        const int slice = threadIdx.x >> 7, which = (threadIdx.x >> 6) & 1, cl = threadIdx.x & 63;
        fin[slice][which][cl] = bn_bwd_slice_sum(partial, slice, R, which, C, cg * 64 + cl);
    }
    __syncthreads();
    if (threadIdx.x < 64) {
        const int cl = threadIdx.x;
        double a = 0.0, b = 0.0;
#pragma unroll
        for (int k = 0; k < 8; ++k) { a += fin[k][0][cl]; b += fin[k][1][cl]; }
        bn_bwd_param_grads(a, b, cg * 64 + cl, dgamma, dbeta, acc);
    }
}

// gy = g' = gz * act'(y)
__global__ void __launch_bounds__(256)
bn_bwd_apply_kernel(const uint4 *__restrict__ gz, const uint4 *__restrict__ y, uint4 *__restrict__ gy, long total8,
                    int act, int dt) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total8; i += (long)gridDim.x * blockDim.x) {
        float g[8], v[8], o[8];
        unpack8(gz[i], g, dt);
        unpack8(y[i], v, dt);
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = act_grad(g[j], v[j], act);
        gy[i] = pack8(o, dt);
    }
}

// bn_bwd_finalize + bn_bwd_apply in one launch (BatchNorm stages): a block owns a 64-channel slice and a pixel range;
// it sums the R <= 128 partial rows of ITS 64 channels (same order and precision as bn_bwd_finalize_kernel: slices of
// 8 rows apart, then the 8 slices, in double), derives the three coefficients, and applies them to its pixels.
// Block (slice, 0) publishes dgamma / dbeta.  One dependent launch (~5 us of pure latency) less per BatchNorm layer
// and backward pass: 150 of them per training window.
__global__ void __launch_bounds__(256)
bn_bwd_finalize_apply_kernel(const float *__restrict__ partial, int R, int C, const float *__restrict__ scale,
                             const float *__restrict__ shift, const float *__restrict__ mean, const float *__restrict__ invstd,
                             float inv_n, float *__restrict__ dgamma, float *__restrict__ dbeta, const uint4 *__restrict__ gz,
                             const uint4 *__restrict__ y, uint4 *__restrict__ gy, long npix, int act, int dt, long pix_per_block,
                             int acc) {
    __shared__ double fin[2][2][64];
    __shared__ float co[3][64], ssc[64], ssh[64];
    const int cg = blockIdx.x, c0 = cg * 64;
    {
        // 256 threads = (group of slices, which, channel): group h sums the slices k = 4h .. 4h+3 of bn_bwd_finalize_kernel's
        // order (slice k = rows k, k+8, k+16, ...), so that (group 0) + (group 1) = its slice-ordered total
        const int cl = threadIdx.x & 63, which = (threadIdx.x >> 6) & 1, h = threadIdx.x >> 7;
        double a = 0.0;
        for (int k = 4 * h; k < 4 * h + 4; ++k) a += bn_bwd_slice_sum(partial, k, R, which, C, c0 + cl);
        fin[h][which][cl] = a;
    }
    __syncthreads();
    if (threadIdx.x < 64) {
        const int cl = threadIdx.x, c = c0 + cl;
        const double a = fin[0][0][cl] + fin[1][0][cl], b = fin[0][1][cl] + fin[1][1][cl];
        bn_bwd_coef(a, b, scale[c], invstd[c], mean[c], inv_n, co[0][cl], co[1][cl], co[2][cl]);
        ssc[cl] = scale[c];
        ssh[cl] = shift[c];
        if (blockIdx.y == 0) bn_bwd_param_grads(a, b, c, dgamma, dbeta, acc);
    }
    __syncthreads();
    const int oc = threadIdx.x & 7, prow = threadIdx.x >> 3;
    float sc[8], sh[8], cA[8], cB[8], cC[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        sc[j] = ssc[oc * 8 + j]; sh[j] = ssh[oc * 8 + j];
        cA[j] = co[0][oc * 8 + j]; cB[j] = co[1][oc * 8 + j]; cC[j] = co[2][oc * 8 + j];
    }
    const int C8 = C >> 3;
    const long p_begin = (long)blockIdx.y * pix_per_block, p_end = min(npix, p_begin + pix_per_block);
    for (long p = p_begin + prow; p < p_end; p += 32 * 4) {
        uint4 gq[4], yq[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long q = min(p + 32 * u, p_end - 1), i = q * C8 + cg * 8 + oc;
            gq[u] = gz[i];
            yq[u] = y[i];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long q = p + 32 * u;
            if (q >= p_end) break;
            gy[q * C8 + cg * 8 + oc] = bn_bwd_gy8(gq[u], yq[u], sc, sh, cA, cB, cC, act, dt);
        }
    }
}

// dx[n][y][x][c] = sum over padded positions (py,px) that reflect onto (y,x) of dxpad[n][py][px][c]
__global__ void __launch_bounds__(256)
fold_reflect_kernel(const uint4 *__restrict__ dxpad, uint4 *__restrict__ dx, int H, int W, int C8, int pady, int padx,
                    long total8, int dt) {
    const int Hp = H + 2 * pady, Wp = W + 2 * padx;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total8; i += (long)gridDim.x * blockDim.x) {
        long r = i;
        const int c8 = (int)(r % C8); r /= C8;
        const int x = (int)(r % W); r /= W;
        const int y = (int)(r % H);
        const long n = r / H;
        // candidate padded rows: y+pad (identity), pad-y (top mirror, 1<=y<=pad), pad+2H-2-y (bottom mirror)
        int ys[3], xs[3], ny = 0, nx = 0;
        ys[ny++] = y + pady;
        if (y >= 1 && y <= pady) ys[ny++] = pady - y;
        if (y <= H - 2 && y >= H - 1 - pady) ys[ny++] = pady + 2 * H - 2 - y;
        xs[nx++] = x + padx;
        if (x >= 1 && x <= padx) xs[nx++] = padx - x;
        if (x <= W - 2 && x >= W - 1 - padx) xs[nx++] = padx + 2 * W - 2 - x;
        float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int a = 0; a < ny; ++a)
            for (int b = 0; b < nx; ++b) {
                float f[8];
                unpack8(dxpad[((n * Hp + ys[a]) * (long)Wp + xs[b]) * C8 + c8], f, dt);
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[j] += f[j];
            }
        dx[i] = pack8(acc, dt);
    }
}

// din[n][ci][y][ix] = sum_{kx, ox : pad(ox*sx + kx - px) == ix} dxe[n][y][ox][ci*KW + kx]   (fp32 NCHW out)
// One thread per input pixel (n, y, ix) and ALL its channels: the <= 3*KW expanded pixels that feed it are 128-byte rows,
// and the Cin values wanted from a row sit in that one row -- one thread per (channel, pixel) fetched every row Cin times
// from waves far apart (84 us for a 512x1024 image at 6 channels; the tensors are 20 us of HBM time).
#define XB_MAXC 32
// f(kx, ox) for every expanded pixel (tap kx of output column ox) that forward filled from input column ix, kx outer
// and the mirror candidates inner: the order both kernels below add in (their sums are bit-identical).
template <class F>
__device__ __forceinline__ void xexpand_sources(int ix, int W, int Wout, int KW, int sx, int px, int pad_mode, F &&f) {
    // unpadded source positions that map to ix: ix itself, and its mirror images under reflection
    int cand[3], nc = 0;
    cand[nc++] = ix;
    if (pad_mode) {
        if (ix >= 1) cand[nc++] = -ix;
        if (ix <= W - 2) cand[nc++] = 2 * W - 2 - ix;
    }
    for (int kx = 0; kx < KW; ++kx)
        for (int q = 0; q < nc; ++q) {
            const int t = cand[q] + px - kx;  // = ox * sx
            if (t < 0 || (t % sx) != 0) continue;
            const int ox = t / sx;
            if (ox >= Wout) continue;
            const int src = ox * sx + kx - px;  // must lie inside the padded range actually read in forward
            if (src < -px || src > W - 1 + px) continue;
            f(kx, ox);
        }
}

__global__ void __launch_bounds__(256)
xexpand_bwd_kernel(const uint16_t *__restrict__ dxe, float *__restrict__ din, int Cin, int H, int W, int Wout, int KW,
                   int sx, int px, int pad_mode, long total, int dt) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        long r = i;
        const int ix = (int)(r % W); r /= W;
        const int y = (int)(r % H);
        const long n = r / H;
        float acc[XB_MAXC];
#pragma unroll
        for (int c = 0; c < XB_MAXC; ++c) acc[c] = 0.f;
        xexpand_sources(ix, W, Wout, KW, sx, px, pad_mode, [&](int kx, int ox) {
            const uint16_t *row = dxe + ((n * H + y) * (long)Wout + ox) * 64 + kx;
#pragma unroll
            for (int c = 0; c < XB_MAXC; ++c)
                if (c < Cin) acc[c] += h2f(row[c * KW], dt);
        });
#pragma unroll
        for (int c = 0; c < XB_MAXC; ++c)
            if (c < Cin) din[((n * Cin + c) * H + y) * (long)W + ix] = acc[c];
    }
}

// The same sum with the expanded rows staged once: one workgroup = one image row (n, y) x XB_TW input columns.  The
// <= XB_TW/sx + KW + 2 px expanded pixels that feed the tile are copied to LDS as whole 128-byte rows (16-byte loads, every
// byte of dxe read once from HBM instead of ~KW times through the caches from scattered 2-byte loads: 78 -> ~25 us for a
// 512x1024 image), then thread (ix, channel parity) gathers its values from LDS in the per-pixel kernel's order (kx outer,
// mirror candidates inner: bit-identical sums).  Rows are pitched 33 dwords apart (consecutive pixels on different banks).
#define XB_TW 128
#define XB_PITCH 33
__global__ void __launch_bounds__(256)
xexpand_bwd_tile_kernel(const uint4 *__restrict__ dxe, float *__restrict__ din, int Cin, int H, int W, int Wout, int KW,
                        int sx, int px, int pad_mode, int xtiles, int dt) {
    extern __shared__ uint32_t xrows[];                    // [rows][XB_PITCH]
    const int xt = blockIdx.x % xtiles;
    const long row = blockIdx.x / xtiles;                  // n*H + y
    const long n = row / H;
    const int y = (int)(row - n * H);
    const int ix0 = xt * XB_TW, tw = min(XB_TW, W - ix0), ixl = ix0 + tw - 1;
    // expanded columns ox with ox*sx in [cand + px - (KW-1), cand + px] for a candidate source column of the tile
    int tlo = ix0 + px - (KW - 1), thi = ixl + px;
    if (pad_mode && ixl >= W - 1 - px && ix0 <= W - 2) thi = max(thi, 2 * W - 2 - max(ix0, W - 1 - px) + px);   // right mirrors
    if (pad_mode && ix0 <= px) tlo = min(tlo, 0);                                                                // left mirrors
    const int oxlo = tlo <= 0 ? 0 : (tlo + sx - 1) / sx;
    const int oxhi = min(Wout - 1, thi / sx);
    const int nrows = oxhi - oxlo + 1;
    const uint4 *src = dxe + (row * Wout + oxlo) * 8;
    for (int i0 = threadIdx.x; i0 < nrows * 8; i0 += 256 * 4) {
        uint4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = src[min(i0 + 256 * u, nrows * 8 - 1)];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + 256 * u;
            if (i < nrows * 8) {
                uint32_t *d = xrows + (i >> 3) * XB_PITCH + (i & 7) * 4;
                d[0] = v[u].x; d[1] = v[u].y; d[2] = v[u].z; d[3] = v[u].w;
            }
        }
    }
    __syncthreads();
    const int il = threadIdx.x & (XB_TW - 1), par = threadIdx.x >> 7;      // channels par, par + 2, ...
    if (il >= tw) return;
    const int ix = ix0 + il;
    float acc[XB_MAXC / 2];
#pragma unroll
    for (int j = 0; j < XB_MAXC / 2; ++j) acc[j] = 0.f;
    xexpand_sources(ix, W, Wout, KW, sx, px, pad_mode, [&](int kx, int ox) {
        const uint32_t *r = xrows + (ox - oxlo) * XB_PITCH;
#pragma unroll
        for (int j = 0; j < XB_MAXC / 2; ++j) {
            const int c = par + 2 * j;
            if (c < Cin) {
                const int e = c * KW + kx;
                const uint32_t w = r[e >> 1];
                acc[j] += h2f((uint16_t)((e & 1) ? (w >> 16) : (w & 0xffff)), dt);
            }
        }
    });
#pragma unroll
    for (int j = 0; j < XB_MAXC / 2; ++j) {
        const int c = par + 2 * j;
        if (c < Cin) din[((n * Cin + c) * H + y) * (long)W + ix] = acc[j];
    }
}

// Gradient of a thin fp32 output (the 1-channel PatchGAN logits, Cout <= 8) prepared for the MFMA kernels in
// one pass: g64 = the gradient as a 64-channel NHWC half tensor (data-gradient operand, channels >= Cout zero),
// g8 = the same in 8 channels (weight-gradient operand), dbias[c] = sum of the fp32 gradient.  Eight lanes
// share a pixel (one 16-byte store each into its 128-byte g64 row); the last Cout blocks reduce one channel
// each in a fixed order.
__global__ void __launch_bounds__(256)
thin_grad_expand_kernel(const float *__restrict__ gz, uint4 *__restrict__ g64, uint4 *__restrict__ g8,
                        float *__restrict__ dbias, long npix, long hw, int Cout, int dt, int expand_blocks) {
    if ((int)blockIdx.x >= expand_blocks) {
        __shared__ float red[256];
        const int c = blockIdx.x - expand_blocks;
        float s = 0.f;
        for (long p = threadIdx.x; p < npix; p += 256 * 8) {      // eight loads in flight (clamped, masked), index order
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const long pp = min(p + 256 * u, npix - 1);
                const long n = pp / hw;
                v[u] = gz[(n * Cout + c) * hw + (pp - n * hw)];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) s += p + 256 * u < npix ? v[u] : 0.f;
        }
        red[threadIdx.x] = s;
        __syncthreads();
        for (int w = 128; w >= 1; w >>= 1) {
            if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
            __syncthreads();
        }
        if (threadIdx.x == 0) dbias[c] = red[0];
        return;
    }
    const long total = npix * 8;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += expand_blocks * 256L) {
        const long p = i >> 3;
        const int o8 = (int)(i & 7);
        uint4 v = make_uint4(0, 0, 0, 0);
        if (o8 == 0) {
            const long n = p / hw, q = p - n * hw;
            float f[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) f[j] = j < Cout ? gz[(n * Cout + j) * hw + q] : 0.f;
            v = pack8(f, dt);
            g8[p] = v;
        }
        g64[i] = v;
    }
}

// R pixel ranges per 64-channel group for bn_bwd_reduce_kernel: about 512 blocks of 512 threads in all, at least 128
// pixels per range and at most 128 ranges (bn_bwd_slice_sum's 8 slices x 16 rows).
static BnChunks bn_bwd_ranges(long npix, int C) { return bn_chunks(npix, C, 512, 8, 128); }

// ----------------------------------------------------------------------------------------
// BatchNorm backward in ONE launch for layers with few pixels (the 1024-channel residual blocks at 32x64, the deep
// discriminator layers: half of the BatchNorm layers of a training window).  The two-launch form above needs the
// per-channel sums of the WHOLE tensor before any gradient can be written, i.e. a kernel boundary between reduce and
// apply; each of the two launches then costs ~13 us of dependent latency on tensors of a few MB.  Here a workgroup owns a
// group of CPB channels over ALL pixels: its slab of gz and y (P x CPB halfs each) fits the registers of 512 threads
// (K 16-byte loads per tensor and thread, all in flight at once; 512 threads leave a thread 256 registers -- at 1024 the
// 128-register cap spilled from K = 4 on, and scratch costs dispatch latency), so it sums, derives the coefficients and
// applies them without the tensors leaving the CU -- one read of gz and y, one write of gy, no partial rows, no second launch.
//   thread t: channel octet t % (CPB/8), pixels t / (CPB/8) + k * (512 / (CPB/8)), k < K
// Sums: per thread in fp32, across the lanes of a wave by shuffles, across the 8 waves in wave order in double.
// ----------------------------------------------------------------------------------------
// (This kernel writes the sums, the coefficients and gy out itself instead of calling bn.h: built from the shared device
// functions it computed the same bits but took 1 % longer at 1024 ch x 32x64 -- 11.20 -> 11.31 us, 30 instructions and
// 5 waits more at K = 4 -- so it keeps the code hipcc schedules best.  Its gy contracts fma(cA, g', cB*y) + cC.)
template <int K, int CPB>
__global__ void __launch_bounds__(512)
bn_bwd_onepass_kernel(const uint4 *__restrict__ gz, const uint4 *__restrict__ y, const float *__restrict__ scale,
                      const float *__restrict__ shift, const float *__restrict__ mean, const float *__restrict__ invstd,
                      uint4 *__restrict__ gy, float *__restrict__ dgamma, float *__restrict__ dbeta, long npix, int C, int act,
                      int dt, float inv_n, int acc, int xcd_remap) {
    constexpr int LPP = CPB / 8;                 // lanes per pixel
    constexpr int PPP = 512 / LPP;               // pixels per pass
    __shared__ double red[2][8][CPB];
    __shared__ float co[3][CPB];
    const int t = threadIdx.x, oc = t % LPP, prow = t / LPP, wave = t >> 6, lane = t & 63;
    // Workgroups whose channel groups share 128-byte lines (64 / CPB neighbours) go to ONE XCD (blockIdx % 8 under
    // round-robin placement): each L2 then fetches a line once and merges the 16-byte stores into whole lines, instead
    // of eight L2s fetching and partially writing every line (speed only: any placement gives the same result).
    // (xcd_remap is always 1; the argument stays because hipcc schedules the kernel differently without it)
    const int G = gridDim.x;
    const int grp = xcd_remap && (G & 7) == 0 ? (int)(blockIdx.x & 7) * (G >> 3) + (int)(blockIdx.x >> 3) : (int)blockIdx.x;
    const int c0 = grp * CPB + oc * 8, C8 = C >> 3;
    const long cidx = (long)grp * LPP + oc;
    uint4 gq[K], yq[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {                // unconditional loads from a clamped pixel, masked below (a predicated
        const long p = (long)prow + (long)k * PPP;   // load compiles to a branch with its own wait: K serial round trips)
        const long q = p < npix ? p : npix - 1;
        gq[k] = gz[q * C8 + cidx];
        yq[k] = y[q * C8 + cidx];
    }
    float sc[8], sh[8], mu[8], is[8], s1[8], s2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { sc[j] = scale[c0 + j]; sh[j] = shift[c0 + j]; mu[j] = mean[c0 + j]; is[j] = invstd[c0 + j]; s1[j] = s2[j] = 0.f; }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const bool ok = (long)prow + (long)k * PPP < npix;
        float g[8], v[8];
        unpack8(gq[k], g, dt);
        unpack8(yq[k], v, dt);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float gp = ok ? act_grad(g[j], v[j] * sc[j] + sh[j], act) : 0.f;
            s1[j] += gp;
            s2[j] += gp * (v[j] - mu[j]) * is[j];
        }
        __builtin_amdgcn_sched_barrier(0);       // (one load's 16 unpacked values at a time: the slab itself stays packed)
    }
    // lanes of a wave that hold the same channel octet: lane bits log2(LPP) .. 5
#pragma unroll
    for (int j = 0; j < 8; ++j) {
#pragma unroll
        for (int m = LPP; m < 64; m <<= 1) {
            s1[j] += __shfl_xor(s1[j], m);
            s2[j] += __shfl_xor(s2[j], m);
        }
    }
    if (lane < LPP) {
#pragma unroll
        for (int j = 0; j < 8; ++j) { red[0][wave][lane * 8 + j] = (double)s1[j]; red[1][wave][lane * 8 + j] = (double)s2[j]; }
    }
    __syncthreads();
    if (t < CPB) {
        double a = 0.0, b = 0.0;
#pragma unroll
        for (int w = 0; w < 8; ++w) { a += red[0][w][t]; b += red[1][w][t]; }
        const int c = grp * CPB + t;
        const float scv = scale[c], isv = invstd[c], muv = mean[c];
        const float dg = (float)b * inv_n, db = (float)a * inv_n;
        co[0][t] = scv;
        co[1][t] = -scv * isv * dg;
        co[2][t] = scv * (isv * muv * dg - db);
        dbeta[c] = (acc ? dbeta[c] : 0.f) + (float)a;
        dgamma[c] = (acc ? dgamma[c] : 0.f) + (float)b;
    }
    __syncthreads();
    float cA[8], cB[8], cC[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { cA[j] = co[0][oc * 8 + j]; cB[j] = co[1][oc * 8 + j]; cC[j] = co[2][oc * 8 + j]; }
    // (the slab stays PACKED between the two passes: without this the compiler keeps the 16 unpacked floats of every
    // load alive across the reduction -- 238 registers at K = 8, scratch beyond)
#pragma unroll
    for (int k = 0; k < K; ++k)
        asm volatile("" : "+v"(gq[k].x), "+v"(gq[k].y), "+v"(gq[k].z), "+v"(gq[k].w), "+v"(yq[k].x), "+v"(yq[k].y), "+v"(yq[k].z), "+v"(yq[k].w));
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const long p = (long)prow + (long)k * PPP;
        float g[8], v[8], o[8];
        unpack8(gq[k], g, dt);
        unpack8(yq[k], v, dt);
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = cA[j] * act_grad(g[j], v[j] * sc[j] + sh[j], act) + cB[j] * v[j] + cC[j];
        if (p < npix) gy[p * C8 + cidx] = pack8(o, dt);
        __builtin_amdgcn_sched_barrier(0);
    }
}

template <int CPB>
static bool bn_bwd_onepass_launch(int K, dim3 grid, hipStream_t s, const uint4 *gz, const uint4 *y, const float *scale,
                                  const float *shift, const float *mean, const float *invstd, uint4 *gy, float *dgamma,
                                  float *dbeta, long npix, int C, int act, int dt, float inv_n, int acc) {
#define IR2RGB_ONEPASS(KK) bn_bwd_onepass_kernel<KK, CPB><<<grid, 512, 0, s>>>(gz, y, scale, shift, mean, invstd, gy, dgamma, dbeta, npix, C, act, dt, inv_n, acc, 1)
    if (K <= 4) IR2RGB_ONEPASS(4);
    else if (K <= 8) IR2RGB_ONEPASS(8);       // (K = 12 would need scratch: 256 registers are gone at K = 9)
    else return false;
#undef IR2RGB_ONEPASS
    return true;
}

extern "C" int ir2rgb_bn_bwd_blocks(long npix, int C) {
    if (npix < 1 || C < 64 || (C & (C - 1)) || C > 2048) return IR2RGB_EINVAL;
    return bn_bwd_ranges(npix, C).n;
}

extern "C" int ir2rgb_bn_bwd(const void *gz, const void *y, const float *scale, const float *shift, const float *mean,
                             const float *invstd, void *gy, float *dgamma, float *dbeta, float *partial, long npix,
                             int C, int act, int dtype, void *stream) {
    const int rc = ir2rgb_bn_bwd_blocks(npix, C);
    if (rc < 0) return rc;
    if (dtype != IR2RGB_BF16 && dtype != IR2RGB_F16) return IR2RGB_ENOSUP;
    const bool frozen = act >= 0 && (act & IR2RGB_BN_BWD_FROZEN);   // evaluation-mode BatchNorm: the mean / variance terms vanish
    const int acc = act >= 0 && (act & IR2RGB_BN_BWD_ACCUMULATE) ? 1 : 0;   // dgamma / dbeta += (a later sample group of a batched forward)
    if (act >= 0) act &= 15;
    if (!gz || !y || !gy || !dgamma || !dbeta || !partial || act < 0 || act > 2) return IR2RGB_EINVAL;
    const bool norm = scale != nullptr;      // a BatchNorm stage hands over all four vectors, a norm-less stage none
    if ((shift != nullptr) != norm || (mean != nullptr) != norm || (invstd != nullptr) != norm) return IR2RGB_EINVAL;
    hipStream_t s = as_stream(stream);
    const uint4 *gz4 = (const uint4 *)gz, *y4 = (const uint4 *)y;
    uint4 *gy4 = (uint4 *)gy;
    const float inv_n = frozen ? 0.f : 1.0f / (float)npix;
    // few pixels per channel: the one-launch form (a workgroup owns CPB channels over all pixels, slabs in registers).
    // 8 channels per workgroup while that gives at most 8 loads per tensor and thread, else not applicable; wider
    // groups (better coalescing, fewer workgroups) when the layer still yields >= 128 workgroups.
    if (norm && !frozen && npix <= 8 * 512) {
        const int min_wg = 128;
        auto onepass = [&](auto cpb) {
            constexpr int CPB = decltype(cpb)::value;
            return bn_bwd_onepass_launch<CPB>((int)((npix * (CPB / 8) + 511) / 512), dim3(C / CPB), s, gz4, y4, scale, shift, mean,
                                              invstd, gy4, dgamma, dbeta, npix, C, act, dtype, inv_n, acc);
        };
        bool done;
        if (C / 32 >= min_wg && npix * 4 <= 8 * 512) done = onepass(std::integral_constant<int, 32>{});
        else if (C / 16 >= min_wg && npix * 2 <= 8 * 512) done = onepass(std::integral_constant<int, 16>{});
        else done = onepass(std::integral_constant<int, 8>{});
        if (done) return ir2rgb_launch_status();
    }
    // partial holds R*2*C floats (and a reserved tail of 3*C, see ir2rgb_hip.h)
    const BnChunks ranges = bn_bwd_ranges(npix, C);
    const int R = ranges.n;
    bn_bwd_reduce_kernel<<<R * (C / 64), 512, 0, s>>>(gz4, y4, scale, shift, mean, invstd, partial, npix, C, act, dtype, ranges.per);
    if (norm) {
        const BnChunks ch = bn_apply_chunks(npix, C);
        bn_bwd_finalize_apply_kernel<<<dim3((unsigned)(C / 64), (unsigned)ch.n), 256, 0, s>>>(
            partial, R, C, scale, shift, mean, invstd, inv_n, dgamma, dbeta, gz4, y4, gy4, npix, act, dtype, ch.per, acc);
        return ir2rgb_launch_status();
    }
    bn_bwd_finalize_kernel<<<C / 64, 1024, 0, s>>>(partial, R, C, dgamma, dbeta, acc);
    const long total8 = npix * (C / 8);
    bn_bwd_apply_kernel<<<stream_grid(total8, 256), 256, 0, s>>>(gz4, y4, gy4, total8, act, dtype);
    return ir2rgb_launch_status();
}

extern "C" int ir2rgb_fold_reflect(const void *dxpad, void *dx, int N, int H, int W, int C, int pad_h, int pad_w,
                                   int dtype, void *stream) {
    if (N < 0 || H < 1 || W < 1 || C < 8 || (C % 8) || pad_h < 0 || pad_w < 0 || pad_h >= H || pad_w >= W)
        return IR2RGB_EINVAL;
    if (dtype != IR2RGB_BF16 && dtype != IR2RGB_F16) return IR2RGB_ENOSUP;
    long total8 = (long)N * H * W * (C / 8);
    if (total8 == 0) return IR2RGB_OK;
    fold_reflect_kernel<<<stream_grid(total8, 256), 256, 0, as_stream(stream)>>>((const uint4 *)dxpad, (uint4 *)dx, H, W,
                                                                                 C / 8, pad_h, pad_w, total8, dtype);
    return ir2rgb_launch_status();
}

extern "C" int ir2rgb_xexpand_bwd(const void *dxe, float *din, int N, int Cin, int H, int W, int Wout, int KW,
                                  int stride_w, int pad_w, int pad_mode, int dtype, void *stream) {
    if (N < 0 || Cin < 1 || H < 1 || W < 1 || Wout < 1 || KW < 1 || Cin * KW > 64 || stride_w < 1 || pad_w < 0)
        return IR2RGB_EINVAL;
    if (dtype != IR2RGB_BF16 && dtype != IR2RGB_F16) return IR2RGB_ENOSUP;
    if (Cin > XB_MAXC) return IR2RGB_ENOSUP;
    long total = (long)N * H * W;
    if (total == 0) return IR2RGB_OK;
    {
        const int xtiles = (W + XB_TW - 1) / XB_TW;
        const long blocks = (long)N * H * xtiles;
        const size_t lds = (size_t)((XB_TW + KW + 2 * pad_w) / stride_w + 3) * XB_PITCH * sizeof(uint32_t);
        if (pad_w < XB_TW && blocks <= 0x7fffffffL && lds <= 64 * 1024 && !((uintptr_t)dxe & 15)) {
            xexpand_bwd_tile_kernel<<<(unsigned)blocks, 256, lds, as_stream(stream)>>>((const uint4 *)dxe, din, Cin, H, W, Wout, KW,
                                                                                    stride_w, pad_w, pad_mode, xtiles, dtype);
            return ir2rgb_launch_status();
        }
    }
    xexpand_bwd_kernel<<<stream_grid(total, 256), 256, 0, as_stream(stream)>>>((const uint16_t *)dxe, din, Cin, H, W, Wout,
                                                                               KW, stride_w, pad_w, pad_mode, total, dtype);
    return ir2rgb_launch_status();
}

extern "C" int ir2rgb_thin_grad_expand(const float *gz, void *g64, void *g8, float *dbias, int N, int Cout, int H, int W,
                                       int dtype, void *stream) {
    if (N < 0 || Cout < 1 || Cout > 8 || H < 1 || W < 1 || !gz || !g64 || !g8 || !dbias) return IR2RGB_EINVAL;
    if (dtype != IR2RGB_BF16 && dtype != IR2RGB_F16) return IR2RGB_ENOSUP;
    if (((uintptr_t)g64 | (uintptr_t)g8) & 15) return IR2RGB_EALIGN;
    const long npix = (long)N * H * W;
    if (npix == 0) return IR2RGB_OK;
    const int eb = stream_grid(npix * 8, 256);
    thin_grad_expand_kernel<<<eb + Cout, 256, 0, as_stream(stream)>>>(gz, (uint4 *)g64, (uint4 *)g8, dbias, npix,
                                                                      (long)H * W, Cout, dtype, eb);
    return ir2rgb_launch_status();
}
