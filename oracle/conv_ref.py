"""fp64 CPU references of the convolution launches of the geometry manifest (test-only).

Every forward-type descriptor (``include/ir2rgb_hip.h`` ``ir2rgb_conv_desc``: plain, reflection-padded, transposed,
adjoint of a reflection pad) is restated as a VALID stride-s convolution of a padded (and, for transposed ones,
zero-dilated) input with an effective [Cout, Cin, kh, kw] weight.  Outputs are evaluated in row bands by im2col + one
fp64 matrix product per band, together with S = the same product on absolute values (the bound's magnitude term,
oracle/bounds.py), so that host memory stays bounded at 512 x 1024.  Results are NHWC ([N, Ho, Wo, C]), the kernels'
pixel order.  Inputs are fp32 tensors holding half-exact values; the products are taken in fp64.
"""
import torch
import torch.nn.functional as F

BAND_ELEMS = 1 << 23            # im2col elements per band (64 MB in fp64)


def act_fn(a):
    return {0: lambda t: t, 1: lambda t: F.leaky_relu(t, 0.2), 2: lambda t: F.leaky_relu(t, 0.1),
            3: torch.relu}[a]


def effective(d, x, w):
    """(xp [N,Cin,Hp,Wp] fp32, weff [Cout,Cin,kh,kw] fp32, stride (sh, sw), fold): the valid convolution equal to the
    launch ``d`` on input ``x`` [N,Cin,H,W] and its weight ``w`` in torch layout ([Cout,Cin,kh,kw] or, transposed /
    adjoint, [Cin,Cout,kh,kw]).  fold: the output is the reflection-padded grid of a pad_mode-2 launch."""
    kh, kw, ph, pw = d["kh"], d["kw"], d["pad_h"], d["pad_w"]
    if d["pad_mode"] == 2:          # data gradient of reflect-pad(1) + 3x3 conv with forward weight w
        weff = w.transpose(0, 1).flip(2, 3)
        return F.pad(x, (kw - 1, kw - 1, kh - 1, kh - 1)), weff, (1, 1), True
    if d["transposed"]:
        sh, sw = d["stride_h"], d["stride_w"]
        n, c, h, wd = x.shape
        xd = x.new_zeros(n, c, (h - 1) * sh + 1, (wd - 1) * sw + 1)
        xd[:, :, ::sh, ::sw] = x
        oph = d["Hout"] - ((h - 1) * sh - 2 * ph + kh)
        opw = d["Wout"] - ((wd - 1) * sw - 2 * pw + kw)
        xp = F.pad(xd, (kw - 1 - pw, kw - 1 - pw + opw, kh - 1 - ph, kh - 1 - ph + oph))
        return xp, w.transpose(0, 1).flip(2, 3), (1, 1), False
    mode = "reflect" if d["pad_mode"] == 1 else "constant"
    xp = F.pad(x, (pw, pw, ph, ph), mode=mode) if (ph or pw) else x
    return xp, w, (d["stride_h"], d["stride_w"]), False


def _bands(ho, wo, k):
    rows = max(1, min(ho, BAND_ELEMS // max(1, k * wo)))
    for o0 in range(0, ho, rows):
        yield o0, min(ho, o0 + rows)


def _cols(xp_n, o0, o1, kh, kw, sh, sw, wo):
    """im2col of output rows [o0, o1) of one sample: [Cin*kh*kw, (o1-o0)*wo] fp64."""
    band = xp_n[:, o0 * sh:(o1 - 1) * sh + kh, :(wo - 1) * sw + kw].unsqueeze(0).double()
    return F.unfold(band, (kh, kw), stride=(sh, sw))[0]


def forward_bands(d, x, w, bias=None):
    """Yields (n, o0, o1, ref, S): fp64 [o1-o0, Wo, Cout] bands of the launch's output (bias and activation included)
    and of its magnitude S.  A pad_mode-2 launch is evaluated whole (it folds borders) as one band per sample."""
    xp, weff, (sh, sw), fold = effective(d, x, w)
    cout, _, kh, kw = weff.shape
    wmat = weff.reshape(cout, -1).double()
    wabs = wmat.abs()
    hp, wp = xp.shape[2], xp.shape[3]
    ho_g, wo_g = (hp - kh) // sh + 1, (wp - kw) // sw + 1
    ho, wo = (ho_g, wo_g) if fold else (d["Hout"], d["Wout"])
    b = bias.double() if bias is not None else None
    act = act_fn(d["act"])
    for n in range(xp.shape[0]):
        bands = [(0, ho)] if fold else _bands(ho, wo, wmat.shape[1])
        for o0, o1 in bands:
            cols = _cols(xp[n], o0, o1, kh, kw, sh, sw, wo)
            ref = (wmat @ cols).T.reshape(o1 - o0, wo, cout)
            S = (wabs @ cols.abs()).T.reshape(o1 - o0, wo, cout)
            if fold:
                ref, S = _fold_reflect(ref), _fold_reflect(S)
                o0, o1 = 0, ref.shape[0]
            if b is not None:
                ref, S = ref + b, S + b.abs()
            yield n, o0, o1, act(ref), S


def _fold_reflect(t):
    """Adjoint of a 1-pixel reflection pad on [H+2, W+2, C] -> [H, W, C]."""
    t = t.clone()
    t[2] += t[0]
    t[-3] += t[-1]
    t[:, 2] += t[:, 0]
    t[:, -3] += t[:, -1]
    return t[1:-1, 1:-1]


def forward(d, x, w, bias=None):
    """Whole fp64 output and magnitude [N, Ho, Wo, Cout] (small geometries)."""
    n = x.shape[0]
    ref = torch.empty(n, d["Hout"], d["Wout"], d["Cout"], dtype=torch.float64)
    S = torch.empty_like(ref)
    for i, o0, o1, r, s in forward_bands(d, x, w, bias):
        ref[i, o0:o1], S[i, o0:o1] = r, s
    return ref, S


def wgrad(d, x, gy):
    """fp64 weight gradient of the launch (torch weight layout) and its magnitude: sum over pixels of gy * x-patch."""
    cout_w = d["Cout"]
    dummy = torch.zeros((d["Cin"], cout_w, d["kh"], d["kw"]) if d["transposed"] else (cout_w, d["Cin"], d["kh"], d["kw"]))
    xp, weff, (sh, sw), fold = effective(d, x, dummy)
    assert not fold
    cout, cin, kh, kw = weff.shape
    ho, wo = d["Hout"], d["Wout"]
    acc = torch.zeros(cout, cin * kh * kw, dtype=torch.float64)
    S = torch.zeros_like(acc)
    for n in range(xp.shape[0]):
        g = gy[n].double().reshape(cout, ho * wo)
        for o0, o1 in _bands(ho, wo, cin * kh * kw):
            cols = _cols(xp[n], o0, o1, kh, kw, sh, sw, wo)
            gb = g[:, o0 * wo:o1 * wo]
            acc += gb @ cols.T
            S += gb.abs() @ cols.abs().T
    acc, S = acc.reshape(cout, cin, kh, kw), S.reshape(cout, cin, kh, kw)
    if d["transposed"]:
        acc, S = acc.flip(2, 3).transpose(0, 1), S.flip(2, 3).transpose(0, 1)
    return acc.contiguous(), S.contiguous()


def draw(shape, gen, scale=1.0):
    """fp32 tensor of bf16 values inside f16's normal range (or 0): exact in both half formats."""
    v = (torch.randn(shape, generator=gen) * scale).to(torch.bfloat16).float()
    v[v.abs() < 2.0 ** -14] = 0
    return v


def weight_shape(d):
    if d["pad_mode"] == 2 or d["transposed"]:
        return (d["Cin"], d["Cout"], d["kh"], d["kw"])
    return (d["Cout"], d["Cin"], d["kh"], d["kw"])


def weight_scale(d):
    taps = d["kh"] * d["kw"]
    if d["transposed"]:
        taps = max(1, taps // (d["stride_h"] * d["stride_w"]))
    return (d["Cin"] * taps) ** -0.5
