"""fp64 restatements of the window's non-convolution entry points (test-only; numpy on the CPU).

Each function restates what include/ir2rgb_hip.h defines, from that definition and the reference formulas it cites --
not from the kernel.  Inputs are fp64 arrays holding the values the kernel reads (fp32 or half values); outputs are
exact fp64 results plus the absolute-value companions ``S`` that the bounds of oracle/bounds.py need.

Layouts follow the header: NCHW fp32 planes, NHWC half buffers with ``ld`` channels per pixel.
"""
import math

import numpy as np


def refl(t, n):
    """nn.ReflectionPad index map (one reflection: |pad| < n)."""
    t = np.abs(t)
    return np.where(t >= n, 2 * n - 2 - t, t)


def nibble(acts, co):
    return (int(acts) >> (4 * co)) & 15


# --------------------------------------------------------------------------------------------------------------------
# layout converters (ir2rgb_nchw_f32_to_nhwc_half[_slice], ir2rgb_nhwc_half_to_nchw_f32)
SLOPE_01 = float(np.float32(0.1))


def nchw_to_nhwc(x, act=0):
    """x [N,C,H,W] fp64 of fp32 values -> [N,H,W,C], what the half store must round.  act 2: LeakyReLU(0.1) -- one fp32
    product x * 0.1f, exact in fp64 (24 + 24 significand bits) and rounded to fp32 here, as F.leaky_relu on the fp32 tensor
    rounds it (FlowNetC.py:32 applies it before any cast): the half store rounds that fp32 value, not the fp64 product."""
    y = x.transpose(0, 2, 3, 1)
    if act == 2:
        y = np.where(y > 0, y, (y * SLOPE_01).astype(np.float32).astype(np.float64))
    return np.ascontiguousarray(y)


# --------------------------------------------------------------------------------------------------------------------
# separable heads (networks.py:166, :170-171, :200-201)
def head_finish(T, bias, Cout, KH, pad, acts, mul):
    """T [N,H,W,CT] -> (out, pre, S_pre) [N,Cout,H,W]: out = f(bias + sum_ky T[refl(y+ky-pad)][x][co*KH+ky])."""
    N, H, W, _ = T.shape
    pre = np.zeros((N, Cout, H, W))
    S = np.zeros((N, Cout, H, W))
    rows = np.arange(H)
    for co in range(Cout):
        b = 0.0 if bias is None else bias[co]
        pre[:, co] = b
        S[:, co] = abs(b)
        for ky in range(KH):
            src = T[..., co * KH + ky][:, refl(rows + ky - pad, H)]
            pre[:, co] += src
            S[:, co] += np.abs(src)
    out = np.empty_like(pre)
    for co in range(Cout):
        a = nibble(acts, co)
        out[:, co] = np.tanh(pre[:, co]) if a == 1 else (1 / (1 + np.exp(-pre[:, co])) if a == 2 else pre[:, co] * mul)
    return out, pre, S


def act_slope(out, acts, mul, Cout):
    """|f'(pre)| per element from the forward output (tanh: 1-o^2, sigmoid: o(1-o), linear: |mul|)."""
    d = np.empty_like(out)
    for co in range(Cout):
        a, o = nibble(acts, co), out[:, co]
        d[:, co] = (1 - o * o) if a == 1 else (o * (1 - o) if a == 2 else abs(mul) + 0 * o)
    return d


def head_finish_bwd(gout, out, Cout, KH, CT, pad, acts, mul):
    """gout/out [N,Cout,H,W] -> dT [N,H,W,CT] (channels >= Cout*KH zero), dbias [Cout], S_dT, S_dbias.
    dpre = gout * f'(pre);  dT[y'][co*KH+ky] = sum over y with refl(y+ky-pad) == y' of dpre[y];  dbias = sum dpre.
    S_* sum the magnitudes the fp32 dpre is formed from (|g|(1+o^2), |g||o|(1+|o|), |g mul|)."""
    N, _, H, W = gout.shape
    dpre = np.empty_like(gout)
    Sd = np.empty_like(gout)
    for co in range(Cout):
        a, o, g = nibble(acts, co), out[:, co], gout[:, co]
        if a == 1:
            dpre[:, co], Sd[:, co] = g * (1 - o * o), np.abs(g) * (1 + o * o)
        elif a == 2:
            dpre[:, co], Sd[:, co] = g * o * (1 - o), np.abs(g * o) * (1 + np.abs(o))
        else:
            dpre[:, co], Sd[:, co] = g * mul, np.abs(g * mul)
    dT = np.zeros((N, H, W, CT))
    S = np.zeros((N, H, W, CT))
    for co in range(Cout):
        for ky in range(KH):
            dst = refl(np.arange(H) + ky - pad, H)
            for y in range(H):
                dT[:, dst[y], :, co * KH + ky] += dpre[:, co, y]
                S[:, dst[y], :, co * KH + ky] += Sd[:, co, y]
    return dT, dpre.sum(axis=(0, 2, 3)), S, Sd.sum(axis=(0, 2, 3))


# --------------------------------------------------------------------------------------------------------------------
# temporal blend (networks.py:89-100, :207-209): grid_sample(bilinear, border, align_corners=False) on the grid
# linspace(-1, 1, W)[x] + flow / ((W-1)/2), i.e. ix = (x + flow_x) * W / (W-1) - 1/2 (the reference's lattice mismatch)
def warp_coords(flow, H, W, align_corners_true=False):
    """flow [N,2,H,W] -> unclamped fp64 (ix, iy).  align_corners_true: the lattice the reference does NOT use."""
    x = np.arange(W)[None, None, :]
    y = np.arange(H)[None, :, None]
    if align_corners_true:
        return x + flow[:, 0], y + flow[:, 1]
    return (x + flow[:, 0]) * W / (W - 1) - 0.5, (y + flow[:, 1]) * H / (H - 1) - 0.5


def _bilinear(prev3, ix, iy, x0=None, y0=None):
    """Border-clamped bilinear samples of prev3 [N,3,H,W] at (ix, iy) [N,H,W] (already clamped).  x0 / y0 override
    the cell (one-sided values at a cell edge).  -> (value [N,3,H,W], d/dix, d/diy, S = sum |p| w)."""
    N, _, H, W = prev3.shape
    x0 = np.floor(ix).astype(np.int64) if x0 is None else x0
    y0 = np.floor(iy).astype(np.int64) if y0 is None else y0
    tx, ty = ix - x0, iy - y0
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    n = np.arange(N)[:, None, None]
    v = np.empty_like(prev3)
    dx = np.empty_like(prev3)
    dy = np.empty_like(prev3)
    S = np.empty_like(prev3)
    for c in range(3):
        pl = prev3[:, c]
        p00, p01, p10, p11 = pl[n, y0, x0], pl[n, y0, x1], pl[n, y1, x0], pl[n, y1, x1]
        v[:, c] = p00 * (1 - tx) * (1 - ty) + p01 * tx * (1 - ty) + p10 * (1 - tx) * ty + p11 * tx * ty
        dx[:, c] = (p01 - p00) * (1 - ty) + (p11 - p10) * ty
        dy[:, c] = (p10 - p00) * (1 - tx) + (p11 - p01) * tx
        S[:, c] = (np.abs(p00) * (1 - tx) * (1 - ty) + np.abs(p01) * tx * (1 - ty) + np.abs(p10) * (1 - tx) * ty +
                   np.abs(p11) * tx * ty)
    return v, dx, dy, S


def warp_blend(raw, prev, flow, w, gout=None, align_corners_true=False, keep_clamped_grad=False, cells=None):
    """Forward (and backward when gout is given) of ir2rgb_warp_blend_*.  raw [N,3,H,W], prev [N,Cp,H,W] (its last 3
    channels are warped), flow [N,2,H,W], w [N,1,H,W].  Returns a dict of fp64 results and their sensitivities:
      out, warp, S_out, dout_dix, dout_diy;  with gout: graw, gw, gflow [N,2,H,W], S_gw, S_gflow, and the derivatives of
      gw / gflow along ix, iy (coordinate-error terms).  The flow gradient is zero where the border clamp is active
      (torch's clip_coordinates_set_grad); keep_clamped_grad leaves it in (a fault).  cells: (x0, y0) override."""
    N, _, H, W = raw.shape
    ix, iy = warp_coords(flow, H, W, align_corners_true)
    inx = (ix > 0) & (ix < W - 1)
    iny = (iy > 0) & (iy < H - 1)
    ixc, iyc = np.clip(ix, 0, W - 1), np.clip(iy, 0, H - 1)
    x0, y0 = cells if cells is not None else (None, None)
    v, dvx, dvy, Sv = _bilinear(prev[:, -3:], ixc, iyc, x0, y0)
    m = w[:, 0][:, None]
    r = {"warp": v, "out": raw * m + v * (1 - m), "S_out": np.abs(raw * m) + Sv * np.abs(1 - m),
         "dout_dix": np.abs((1 - m) * dvx), "dout_diy": np.abs((1 - m) * dvy), "ix": ix, "iy": iy,
         "S_warp": Sv, "dwarp_dix": np.abs(dvx), "dwarp_diy": np.abs(dvy)}
    if gout is None:
        return r
    r["graw"] = gout * m
    r["gw"] = (gout * (raw - v)).sum(1, keepdims=True)
    r["S_gw"] = (np.abs(gout) * (np.abs(raw) + Sv)).sum(1, keepdims=True)
    r["dgw_dix"] = np.abs((gout * dvx).sum(1, keepdims=True))
    r["dgw_diy"] = np.abs((gout * dvy).sum(1, keepdims=True))
    gwarp = gout * (1 - m)
    sx, sy = W / (W - 1), H / (H - 1)
    kx = sx if keep_clamped_grad else np.where(inx, sx, 0.0)
    ky = sy if keep_clamped_grad else np.where(iny, sy, 0.0)
    gfx, gfy = (gwarp * dvx).sum(1), (gwarp * dvy).sum(1)
    r["gflow"] = np.stack([gfx * kx, gfy * ky], 1)
    # |d gfx / d iy| and |d gfy / d ix| (bilinear: gfx is linear in ty, gfy in tx; d gfx/d ix = 0 inside a cell)
    a = np.abs(gwarp)
    pl = prev[:, -3:]
    n = np.arange(N)[:, None, None]
    xa = np.floor(ixc).astype(np.int64) if x0 is None else x0
    ya = np.floor(iyc).astype(np.int64) if y0 is None else y0
    xb, yb = np.minimum(xa + 1, W - 1), np.minimum(ya + 1, H - 1)
    tx, ty = ixc - xa, iyc - ya
    c4 = [[np.abs(pl[:, c][n, yy, xx]) for yy, xx in ((ya, xa), (ya, xb), (yb, xa), (yb, xb))] for c in range(3)]
    sgx = sum(a[:, c] * ((q[0] + q[1]) * (1 - ty) + (q[2] + q[3]) * ty) for c, q in enumerate(c4))
    sgy = sum(a[:, c] * ((q[0] + q[2]) * (1 - tx) + (q[1] + q[3]) * tx) for c, q in enumerate(c4))
    r["S_gflow"] = np.stack([sgx * sx, sgy * sy], 1)
    cross = np.stack([pl[:, c][n, yb, xb] - pl[:, c][n, yb, xa] - pl[:, c][n, ya, xb] + pl[:, c][n, ya, xa]
                      for c in range(3)], 1)
    r["dgflow_x_diy"] = np.abs((gwarp * cross).sum(1)) * sx
    r["dgflow_y_dix"] = np.abs((gwarp * cross).sum(1)) * sy
    return r


# --------------------------------------------------------------------------------------------------------------------
# FlowNet2 resample2d (resample2d_kernel.cu:15-64): pixel-space flow, corners clamped into the image, weights from
# xf - floor(xf) unclamped; then diff = img1 - warped and the channel L2 norm
def resample2d(img, flow):
    """img [N,C,H,W], flow [N,2,H,W] -> (warped, |d/dxf|, |d/dyf|, S = sum |p| w)."""
    N, C, H, W = img.shape
    xf = np.arange(W)[None, None, :] + flow[:, 0]
    yf = np.arange(H)[None, :, None] + flow[:, 1]
    fx, fy = np.floor(xf), np.floor(yf)
    a, b = xf - fx, yf - fy
    xL, xR = np.clip(fx, 0, W - 1).astype(np.int64), np.clip(fx + 1, 0, W - 1).astype(np.int64)
    yT, yB = np.clip(fy, 0, H - 1).astype(np.int64), np.clip(fy + 1, 0, H - 1).astype(np.int64)
    n = np.arange(N)[:, None, None]
    v, dx, dy, S = (np.empty_like(img) for _ in range(4))
    for c in range(C):
        pl = img[:, c]
        tl, tr, bl, br = pl[n, yT, xL], pl[n, yT, xR], pl[n, yB, xL], pl[n, yB, xR]
        v[:, c] = (1 - a) * (1 - b) * tl + a * (1 - b) * tr + (1 - a) * b * bl + a * b * br
        dx[:, c] = np.abs((tr - tl) * (1 - b) + (br - bl) * b)
        dy[:, c] = np.abs((bl - tl) * (1 - a) + (br - tr) * a)
        S[:, c] = (1 - a) * (1 - b) * np.abs(tl) + a * (1 - b) * np.abs(tr) + (1 - a) * b * np.abs(bl) + a * b * np.abs(br)
    return v, dx, dy, S


# --------------------------------------------------------------------------------------------------------------------
# AvgPool2d(3, stride 2, padding 1, count_include_pad=False)
def avgpool_divisors(n):
    """Taps per output along one dimension of size n (2 or 3; 1 when n == 1)."""
    no = (n - 1) // 2 + 1
    o = np.arange(no)
    return np.minimum(2 * o + 1, n - 1) - np.maximum(2 * o - 1, 0) + 1


def avgpool3s2(x, count_include_pad=False):
    """x [P,H,W] -> (y [P,Ho,Wo], S).  count_include_pad=True: a fault (always divides by 9)."""
    P, H, W = x.shape
    xp = np.pad(x, ((0, 0), (1, 2), (1, 2)))
    ap = np.abs(xp)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    s = np.zeros((P, Ho, Wo))
    S = np.zeros((P, Ho, Wo))
    for dy in range(3):
        for dx in range(3):
            s += xp[:, dy:dy + 2 * Ho:2, dx:dx + 2 * Wo:2]
            S += ap[:, dy:dy + 2 * Ho:2, dx:dx + 2 * Wo:2]
    div = 9.0 if count_include_pad else avgpool_divisors(H)[:, None] * avgpool_divisors(W)[None, :]
    return s / div, S / div


def avgpool3s2_bwd(gy, H, W, count_include_pad=False):
    """Adjoint of avgpool3s2: gy [P,Ho,Wo] -> (gx [P,H,W], S)."""
    P, Ho, Wo = gy.shape
    div = 9.0 if count_include_pad else avgpool_divisors(H)[:, None] * avgpool_divisors(W)[None, :]
    q = gy / div
    gp = np.zeros((P, H + 3, W + 3))
    Sp = np.zeros((P, H + 3, W + 3))
    for dy in range(3):
        for dx in range(3):
            gp[:, dy:dy + 2 * Ho:2, dx:dx + 2 * Wo:2] += q
            Sp[:, dy:dy + 2 * Ho:2, dx:dx + 2 * Wo:2] += np.abs(q)
    return gp[:, 1:H + 1, 1:W + 1], Sp[:, 1:H + 1, 1:W + 1]


# --------------------------------------------------------------------------------------------------------------------
# FlowNet2 flow up-sampler ConvTranspose2d(2, 2, 4, stride 2, padding 1)
def flow_upsample(x, w, bias, swap_ky_parity=False):
    """x [N,2,h,w], w [2,2,4,4] (ConvTranspose2d layout [cin][cout][ky][kx]) -> (y [N,2,2h,2w], S).
    y[oy][ox] = bias + sum x[iy][ix] w[ky][kx] over oy = 2 iy - 1 + ky, ox = 2 ix - 1 + kx.
    swap_ky_parity: a fault (rows take the other parity's taps)."""
    N, _, h, wd = x.shape
    y = np.zeros((N, 2, 2 * h + 2, 2 * wd + 2))
    S = np.zeros_like(y)
    for ky in range(4):
        kyw = ky ^ 1 if swap_ky_parity else ky
        for kx in range(4):
            for ci in range(2):
                for co in range(2):
                    # output row 2 iy - 1 + ky -> padded row 2 iy + ky
                    y[:, co, ky:ky + 2 * h:2, kx:kx + 2 * wd:2] += x[:, ci] * w[ci, co, kyw, kx]
                    S[:, co, ky:ky + 2 * h:2, kx:kx + 2 * wd:2] += np.abs(x[:, ci] * w[ci, co, kyw, kx])
    y, S = y[:, :, 1:2 * h + 1, 1:2 * wd + 1], S[:, :, 1:2 * h + 1, 1:2 * wd + 1]
    if bias is not None:
        y = y + bias[None, :, None, None]
        S = S + np.abs(bias)[None, :, None, None]
    return y, S


# --------------------------------------------------------------------------------------------------------------------
# x-direction im2col of the first layers and its adjoint
def xexpand_index(W, Wout, KW, stride, pad, pad_mode):
    """[Wout, KW] source column of out[.., ox, ci*KW + kx] (-1: zero padding)."""
    t = np.arange(Wout)[:, None] * stride + np.arange(KW)[None, :] - pad
    if pad_mode == 1:
        return refl(t, W)
    return np.where((t >= 0) & (t < W), t, -1)


def xexpand(x, Wout, KW, stride, pad, pad_mode, Cx):
    """x [N,Cin,H,W] -> [N,H,Wout,Cx] (channels >= Cin*KW zero)."""
    N, Cin, H, W = x.shape
    idx = xexpand_index(W, Wout, KW, stride, pad, pad_mode)
    xp = np.concatenate([x, np.zeros((N, Cin, H, 1))], axis=3)           # column -1 -> the zero column
    g = xp[:, :, :, idx]                                                  # [N,Cin,H,Wout,KW]
    out = np.zeros((N, H, Wout, Cx))
    out[..., :Cin * KW] = g.transpose(0, 2, 3, 1, 4).reshape(N, H, Wout, Cin * KW)
    return out


def xexpand_bwd(dxe, Cin, W, KW, stride, pad, pad_mode):
    """Adjoint: dxe [N,H,Wout,>=Cin*KW] -> (din [N,Cin,H,W], count of terms per element)."""
    N, H, Wout, _ = dxe.shape
    idx = xexpand_index(W, Wout, KW, stride, pad, pad_mode)
    din = np.zeros((N, Cin, H, W + 1))
    cnt = np.zeros(W + 1)
    g = dxe[..., :Cin * KW].reshape(N, H, Wout, Cin, KW).transpose(0, 3, 1, 2, 4)   # [N,Cin,H,Wout,KW]
    for ox in range(Wout):
        for kx in range(KW):
            din[..., idx[ox, kx]] += g[..., ox, kx]
            cnt[idx[ox, kx]] += 1
    return din[..., :W], cnt[:W]


def fold_reflect(dxpad, pad_h, pad_w):
    """Adjoint of ReflectionPad2d: dxpad [N,H+2ph,W+2pw,C] -> (dx [N,H,W,C], terms per element [H,W])."""
    N, Hp, Wp, C = dxpad.shape
    H, W = Hp - 2 * pad_h, Wp - 2 * pad_w
    ry = refl(np.arange(Hp) - pad_h, H)
    rx = refl(np.arange(Wp) - pad_w, W)
    dx = np.zeros((N, H, W, C))
    cnt = np.zeros((H, W))
    for py in range(Hp):
        rows = np.zeros((N, W, C))
        np.add.at(rows, (slice(None), rx), dxpad[:, py])
        dx[:, ry[py]] += rows
        np.add.at(cnt[ry[py]], rx, 1)
    return dx, cnt


# --------------------------------------------------------------------------------------------------------------------
# grouped losses (losses.hip, the header's kinds 0 / 1 / 2)
def loss_term(kind, a, b, mask, target, hw, chw):
    """Per-element terms and their S (|term| with the products it is formed from)."""
    if kind == 0:
        t = np.abs(a - b)
        return t, np.abs(a) + np.abs(b)
    if kind == 1:
        d = a - target
        return d * d, (np.abs(a) + abs(target)) ** 2
    img = np.arange(a.size) // chw
    m = mask.reshape(-1)[img * hw + np.arange(a.size) % hw]
    bb = 0.0 if b is None else b
    return np.abs(a * m - bb * m), np.abs(a * m) + np.abs(bb * m)


def loss_grad(kind, a, b, mask, target, hw, chw, g):
    """d (weight mean term) / d a scaled by gout, with g = gout * weight / n."""
    if kind == 0:
        return np.sign(a - b) * g
    if kind == 1:
        return 2 * (a - target) * g
    img = np.arange(a.size) // chw
    m = mask.reshape(-1)[img * hw + np.arange(a.size) % hw]
    bb = 0.0 if b is None else b
    return np.sign(a * m - bb * m) * g * m


# --------------------------------------------------------------------------------------------------------------------
# torch.optim.Adam (weight_decay 0, amsgrad off) from the same fp32 p, g, m, v
def adam(p, g, m, v, lr, beta1, beta2, eps, step, bias_correction=True):
    """-> (p', m', v', |update|, S_m, step_size, denom).  beta1 / beta2 are the fp32 values the kernel receives."""
    m1 = beta1 * m + (1 - beta1) * g
    v1 = beta2 * v + (1 - beta2) * g * g
    bc1 = 1 - beta1 ** step if bias_correction else 1.0
    bc2 = 1 - beta2 ** step if bias_correction else 1.0
    step_size = lr / bc1
    denom = np.sqrt(v1) / math.sqrt(bc2) + eps
    upd = step_size * m1 / denom
    return p - upd, m1, v1, np.abs(upd), np.abs(beta1 * m) + np.abs((1 - beta1) * g), step_size, denom
