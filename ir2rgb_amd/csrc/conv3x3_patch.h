// conv3x3_patch.h -- entry points of conv3x3_patch.hip (called from conv_mfma.hip's dispatcher)
#pragma once
#include "common.h"

struct P3Geom {
    int N, H, W, Ho, Wo, Cin, Cout;   // input / output extents
    int pad, pad_mode, act;
    int ldx, ci_off, ldy, co_off;
    int stats_row0, nty, ntx;         // pixel tiles per image: nty x ntx
    int cout_major, kchunks;
    unsigned x_bytes, w_bytes;
    int dbg;                          // always 0; conv3x3_patch_kernel still tests it (without the tests hipcc reschedules every form of it)
};

// variant: 0 = not applicable, 1 = 2x64 px x 64 cout, 2 = 2x128 px x 128 cout, 3, 4 = split-K forms (allow_split only)
int conv3x3p_plan(const ir2rgb_conv_desc *d, const ConvView &v, P3Geom *g, int *npt_out, bool allow_split);
long conv3x3p_workspace_bytes(int variant, const P3Geom &g);
int conv3x3p_launch(int variant, const P3Geom &g, int dtype, const void *x, const void *wp, const float *bias, void *y,
                    float *stats, hipStream_t s, void *workspace, long workspace_bytes);
