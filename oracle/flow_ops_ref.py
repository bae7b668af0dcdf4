"""fp64 references of the FlowNet2 operators (test-only, numpy on the CPU): the cost volume and its gradients, the
gradients of the pixel-space warp, the gradient of the channel norm.  Like oracle/window_ops_ref.py each returns the
value and ``S``, the same operation on absolute values, for the bounds of oracle/bounds.py.  Nothing here loads the
library.  Semantics: include/ir2rgb_hip.h and the kernels' comments (correlation.hip, resample2d.hip, channelnorm.hip).
"""
import numpy as np

from oracle import window_ops_ref as O


def correlation_out_shape(H, W, pad, k, md, s1, s2):
    border = (k - 1) // 2 + md
    d = md // s2
    return (2 * d + 1) ** 2, -(-(H + 2 * pad - 2 * border) // s1), -(-(W + 2 * pad - 2 * border) // s1)


def _corr_banded(f1, f2, md, s2):
    """k = 1, stride1 = 1, pad = md: out[n, tj, ti, y, x] = sum_c f1[n,c,y,x] f2[n,c,y + s2 tj, x + s2 ti].  x and
    x + s2 ti are congruent mod s2, so per displacement row tj and residue r the 2d + 1 values of a pixel lie on the
    diagonals -d .. d of one matrix product over the channels: (W / s2)^2 C flops for 2d + 1 outputs."""
    N, C, H, W = f1.shape
    d = md // s2
    D = 2 * d + 1
    out = np.zeros((N, D, D, H, W), dtype=f1.dtype)
    res = range(min(s2, W))
    a = [np.ascontiguousarray(f1[..., r::s2].transpose(0, 2, 3, 1)) for r in res]       # [N, H, i, C]
    b = [np.ascontiguousarray(f2[..., r::s2].transpose(0, 2, 1, 3)) for r in res]       # [N, H, C, j]
    for tj in range(-d, d + 1):
        y0, y1 = max(0, -tj * s2), min(H, H - tj * s2)
        if y0 >= y1:
            continue
        for r in res:
            M = np.matmul(a[r][:, y0:y1], b[r][:, y0 + tj * s2:y1 + tj * s2])            # [N, Y, i, j]
            n = M.shape[-1]
            for ti in range(max(-d, 1 - n), min(d, n - 1) + 1):
                i0, i1 = max(0, -ti), min(n, n - ti)
                out[:, tj + d, ti + d, y0:y1, r + s2 * i0:r + s2 * i1:s2] = np.diagonal(M, ti, -2, -1)
    return out.reshape(N, D * D, H, W)


def _corr_general(f1, f2, pad, k, md, s1, s2, clamp_border=False):
    """Any parameters: per displacement and window tap, the product of two index-gathered planes (zero where either
    index leaves the image; ``clamp_border``, a fault: the border pixel repeated instead)."""
    N, C, H, W = f1.shape
    kr, d = (k - 1) // 2, md // s2
    D = 2 * d + 1
    _, oh, ow = correlation_out_shape(H, W, pad, k, md, s1, s2)
    out = np.zeros((N, D, D, oh, ow), dtype=f1.dtype)
    y1 = np.arange(oh) * s1 + md - pad
    x1 = np.arange(ow) * s1 + md - pad

    def take(f, ys, xs):
        ok = ((ys >= 0) & (ys < H))[:, None] & ((xs >= 0) & (xs < W))[None, :]
        return f[:, :, np.clip(ys, 0, H - 1)][:, :, :, np.clip(xs, 0, W - 1)] * (ok | clamp_border)
    for j in range(-kr, kr + 1):
        for i in range(-kr, kr + 1):
            p1 = take(f1, y1 + j, x1 + i)
            for tj in range(-d, d + 1):
                for ti in range(-d, d + 1):
                    out[:, tj + d, ti + d] += (p1 * take(f2, y1 + j + tj * s2, x1 + i + ti * s2)).sum(1)
    return out.reshape(N, D * D, oh, ow)


def correlation(f1, f2, pad, k, md, s1, s2, clamp_border=False):
    """f1, f2 [N,C,H,W] -> (out [N,(2d+1)^2,outH,outW], S): the mean over the k x k window and the channels of
    f1[y1 + j, x1 + i] * f2[y1 + j + s2 tj, x1 + i + s2 ti], y1 = oy * s1 + md - pad, zero outside the image.  The
    FlowNetC form (k = 1, stride1 = 1, pad = md) runs as banded matrix products.  The arithmetic is the operands' dtype
    (float32 operands give a float32 evaluation, for the order tests)."""
    fn = (lambda a, b: _corr_banded(a, b, md, s2)) if (k == 1 and s1 == 1 and pad == md and not clamp_border) else \
        (lambda a, b: _corr_general(a, b, pad, k, md, s1, s2, clamp_border))
    scale = f1.dtype.type(1.0 / (k * k * f1.shape[1]))
    return fn(f1, f2) * scale, fn(np.abs(f1), np.abs(f2)) * scale


def correlation_bwd(f1, f2, gout, pad, k, md, s2):
    """stride1 = 1.  -> (gin1, gin2, S1, S2, L1, L2) with the windows of corr_bwd_kernel (correlation.hip,
    oracle/ops_ref.c): in padded coordinates (y, x) = (by + pad, bx + pad),

      gin1[n,c,by,bx] = 1/(k^2 C) sum_tc f2[n,c,by + j2,bx + i2] * sum of gout[n,tc] over [y-kr-md, y+kr-md] x [x-kr-md, x+kr-md]
      gin2[n,c,by,bx] = 1/(k^2 C) sum_tc f1[n,c,by - j2,bx - i2] * sum of gout[n,tc] over the same window moved by (-j2, -i2)

    both windows cut to the output and a term absent where the other image's pixel lies outside it.  At stride1 = 1
    this is the autograd adjoint of ``correlation`` for every (pad, k, md, s2) (tests/test_edge_flow_cpu.py compares
    the two); at stride1 > 1 the library refuses, so nothing is pinned there.  L1 / L2: the (tc, window element)
    products of an element."""
    N, C, H, W = f1.shape
    kr, d = (k - 1) // 2, md // s2
    D = 2 * d + 1
    oh, ow = gout.shape[2:]
    ag = np.abs(gout)
    # inclusive prefix sums with a leading zero: a window sum is four look-ups
    P = np.zeros((N, D * D, oh + 1, ow + 1))
    P[:, :, 1:, 1:] = gout.cumsum(2).cumsum(3)
    PA = np.zeros_like(P)
    PA[:, :, 1:, 1:] = ag.cumsum(2).cumsum(3)

    def window(lo_y, lo_x):
        """Sums of gout / |gout| per tc over [lo, lo + 2 kr] cut to the output, for vectors of lower corners; -> also the
        element count."""
        y0, y1 = np.clip(lo_y, 0, oh), np.clip(lo_y + 2 * kr + 1, 0, oh)
        x0, x1 = np.clip(lo_x, 0, ow), np.clip(lo_x + 2 * kr + 1, 0, ow)
        cnt = np.maximum(y1 - y0, 0)[:, None] * np.maximum(x1 - x0, 0)[None, :]

        def box(Q):
            return (Q[:, :, y1][:, :, :, x1] - Q[:, :, y0][:, :, :, x1] - Q[:, :, y1][:, :, :, x0] + Q[:, :, y0][:, :, :, x0])
        return box(P), box(PA), cnt
    by, bx = np.arange(H), np.arange(W)
    g1, g2, S1, S2 = (np.zeros((N, C, H, W)) for _ in range(4))
    L1, L2 = np.zeros((H, W)), np.zeros((H, W))
    w1, wa1, c1 = window(by + pad - kr - md, bx + pad - kr - md)
    for tj in range(-d, d + 1):
        for ti in range(-d, d + 1):
            tc = (tj + d) * D + ti + d
            j2, i2 = tj * s2, ti * s2
            for sign, f, g, S, L in ((1, f2, g1, S1, L1), (-1, f1, g2, S2, L2)):
                if sign == 1:
                    w, wa, cnt = w1, wa1, c1
                else:
                    w, wa, cnt = window(by + pad - kr - md - j2, bx + pad - kr - md - i2)
                ys, xs = by + sign * j2, bx + sign * i2
                ok = ((ys >= 0) & (ys < H))[:, None] & ((xs >= 0) & (xs < W))[None, :]
                v = f[:, :, np.clip(ys, 0, H - 1)][:, :, :, np.clip(xs, 0, W - 1)] * ok
                g += v * w[:, tc][:, None]
                S += np.abs(v) * wa[:, tc][:, None]
                L += cnt * ok
    sc = 1.0 / (k * k * C)
    return g1 * sc, g2 * sc, S1 * sc, S2 * sc, L1, L2


def pixel_coords(flow):
    """xf = (float)x + dx, yf = (float)y + dy as the operator forms them: one fp32 addition each (returned as fp64)."""
    N, _, H, W = flow.shape
    f = flow.astype(np.float32)
    xf = np.arange(W, dtype=np.float32)[None, None, :] + f[:, 0]
    yf = np.arange(H, dtype=np.float32)[None, :, None] + f[:, 1]
    return xf.astype(np.float64), yf.astype(np.float64)


def resample2d_bwd(img, flow, gout, fault=None):
    """-> dict.  Corners as in the forward (floor, indices clamped).  ``fault`` (image gradient only): "floor" (floor
    weights), "corner" (the bottom-right corner dropped), ("lose", flat pixel index) (that pixel's top-left contribution lost).

    gimg / S_gimg / L: every pixel adds gout times (1-a)(1-b), a(1-b), (1-a)b, ab to its four corners, with the
    reference's quirk a = xf - trunc(xf), b = yf - trunc(yf) (negative below zero, where both corners of an axis clamp
    onto the border pixel).  The coordinates here are the operator's own fp32 sums (pixel_coords): the weights are then
    defined exactly and the bound needs no coordinate term.  L counts the contributions of an element (a pixel whose two
    corners coincide contributes twice).
    gflow / S_gflow: floor weights alpha, beta on exact fp64 coordinates,
      gflow_x = sum_c gout ((1 - beta)(tr - tl) + beta (br - bl)),  gflow_y = sum_c gout ((1 - alpha)(bl - tl) + alpha (br - tr)),
    and dgx_dy / dgy_dx, the magnitudes of their derivatives in the other coordinate (for the coordinate terms)."""
    N, C, H, W = img.shape
    n = np.arange(N)[:, None, None]

    def corners(xf, yf):
        fx, fy = np.floor(xf), np.floor(yf)
        return (np.clip(fx, 0, W - 1).astype(np.int64), np.clip(fx + 1, 0, W - 1).astype(np.int64),
                np.clip(fy, 0, H - 1).astype(np.int64), np.clip(fy + 1, 0, H - 1).astype(np.int64), xf - fx, yf - fy)
    # image gradient
    xf, yf = pixel_coords(flow)
    xL, xR, yT, yB, _, _ = corners(xf, yf)
    a, b = (xf - np.trunc(xf), yf - np.trunc(yf)) if fault != "floor" else (xf - np.floor(xf), yf - np.floor(yf))
    gimg, S, L = np.zeros((N, C, H, W)), np.zeros((N, C, H, W)), np.zeros((N, H, W))
    wTL = (1 - a) * (1 - b)
    if isinstance(fault, tuple):
        wTL.reshape(-1)[fault[1]] = 0
    for yy, xx, w in ((yT, xL, wTL), (yT, xR, a * (1 - b)), (yB, xL, (1 - a) * b), (yB, xR, a * b * (fault != "corner"))):
        idx = ((n * H + yy) * W + xx).ravel()
        L += np.bincount(idx, minlength=N * H * W).reshape(N, H, W)
        for c in range(C):
            t = (w * gout[:, c]).ravel()
            gimg[:, c] += np.bincount(idx, weights=t, minlength=N * H * W).reshape(N, H, W)
            S[:, c] += np.bincount(idx, weights=np.abs(t), minlength=N * H * W).reshape(N, H, W)
    # flow gradient
    xf = np.arange(W)[None, None, :] + flow[:, 0]
    yf = np.arange(H)[None, :, None] + flow[:, 1]
    xL, xR, yT, yB, al, be = corners(xf, yf)
    gflow, Sg = np.zeros((N, 2, H, W)), np.zeros((N, 2, H, W))
    dgx_dy, dgy_dx = np.zeros((N, H, W)), np.zeros((N, H, W))
    for c in range(C):
        pl, go = img[:, c], gout[:, c]
        tl, tr, bl, br = pl[n, yT, xL], pl[n, yT, xR], pl[n, yB, xL], pl[n, yB, xR]
        gflow[:, 0] += go * ((1 - be) * (tr - tl) + be * (br - bl))
        gflow[:, 1] += go * ((1 - al) * (bl - tl) + al * (br - tr))
        Sg[:, 0] += np.abs(go) * ((1 - be) * (np.abs(tr) + np.abs(tl)) + be * (np.abs(br) + np.abs(bl)))
        Sg[:, 1] += np.abs(go) * ((1 - al) * (np.abs(bl) + np.abs(tl)) + al * (np.abs(br) + np.abs(tr)))
        cross = go * (br - bl - tr + tl)
        dgx_dy += cross
        dgy_dx += cross
    return {"gimg": gimg, "S_gimg": S, "L": L, "gflow": gflow, "S_gflow": Sg, "dgx_dy": np.abs(dgx_dy), "dgy_dx": np.abs(dgy_dx)}


def resample2d(img, flow):
    """The forward: oracle/window_ops_ref.py's."""
    return O.resample2d(img, flow)


def channelnorm(x):
    return np.sqrt((x * x).sum(1, keepdims=True))


def channelnorm_bwd(x, out, gout):
    """gin = gout * x / (out + 1e-9), ``out`` [N,1,H,W] an input (the forward's stored result).  -> (gin, S = |gin|)."""
    g = gout * x / (out + 1e-9)
    return g, np.abs(g)
