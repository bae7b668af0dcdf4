"""Writes tests/golden/conv_routes.json: what the host queries of libir2rgb_hip.so answer for a fixed list of convolution
descriptors.  No GPU is involved: every call below returns before a launch.

    python tests/golden/make_route_goldens.py            # rewrites the table from the built library

The table is recorded BEFORE a change to the dispatch code of ir2rgb_amd/csrc/ (conv_mfma.hip, wgrad_mfma.hip and the
*_plan functions of the three special kernels) and committed unchanged with it; tests/test_conv_route_cpu.py holds the
library to it row by row and rebuilds the descriptor list from descriptors() below, so neither side can shrink silently.
The environment switches IR2RGB_CONV3X3P, IR2RGB_CONV3X3P_SPLIT and IR2RGB_CONV_DOT must be unset.

The list:
* every distinct convolution descriptor of tests/window_geometries.json, EDGE_CONV and EDGE_WGRAD, in both element types;
* a grid on both sides of every threshold of the dispatch (the functions below, one per threshold group);
* invalid descriptors for every error return.

A row is [kernel name index, stats_rows, packed_weight_elems, fwd_workspace_bytes, wgrad_workspace_elems,
wgrad_acc_workspace_elems, return code of ir2rgb_conv2d_wgrad with a misaligned x (the descriptor's own error, else
IR2RGB_EALIGN -- it returns before any launch), index into "pack"].  A "pack" record holds, for the four single-job
tables (forward and adjoint, each with a 16-byte aligned pointer pair and with w four bytes off), either the error code
or [table bytes, entries, blocks, sha1 of the table ir2rgb_conv2d_pack_batch_build writes].
"""
import ctypes
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import edge_records as ER  # noqa: E402
from oracle.window import DESC_FIELDS  # noqa: E402

PATH = os.path.join(HERE, "conv_routes.json")
NAMES = ("conv_igemm_kernel", "conv_igemm_classes_kernel", "conv_dot_kernel", "conv3x3_patch_kernel",
         "conv1x7_thin_kernel", "conv7x1_col_kernel", "")
BF16, F16 = 1, 2
W_PTR, WP_PTR = 0x10000, 0x20000        # never dereferenced: the table only stores them
PACK_JOBS = ((0, 0), (0, 4), (1, 0), (1, 4))    # (adjoint, byte offset of w)

G = ER.geometry


def _recorded():
    """The convolution descriptors of the window manifest and of the edge records."""
    with open(os.path.join(ROOT, "tests", "window_geometries.json")) as f:
        launches = json.load(f)["launches"]
    return [r["desc"] for r in launches if r["kind"] == "conv"] + [r["desc"] for r in ER.EDGE_CONV + ER.EDGE_WGRAD]


def _tile_pixels():
    """tile_pixels: 255 / 256 tiles of 256 and of 128 pixels at one and at eight channel tiles, 39 / 40 K-steps."""
    out = []
    for Cout, ps in ((1024, (3968, 3969, 7936, 7937)), (1000, (3969, 7937)), (128, (32640, 32641, 65280, 65281))):
        for P in ps:
            for Cin in (64, 2496, 2560):
                out.append(G(1, Cin, 1, P, Cout, 1))
    for k in ((6, 6), (5, 8), (7, 7)):          # 36, 40 and 49 K-steps at Cin = 64
        for P in (7936, 7937):
            out.append(G(1, 64, 1 + k[0] - 1, P + k[1] - 1, 1024, k))
    return out


def _classes():
    """make_plan's sub-pixel classes: tp_all through tile_pixels, wg128 <= 320, mean K-steps 38 / 40."""
    out = []
    for H, W in ((31, 32), (31, 33), (32, 32), (35, 36), (36, 36), (36, 37), (45, 44), (45, 45)):
        for op in (0, 1):
            for Cin, Cout in ((64, 1024), (64, 512), (1088, 1024), (1152, 1024)):
                out.append(G(1, Cin, H, W, Cout, 3, stride=2, pad=1, transposed=1, output_padding=op))
    for H, W in ((5, 7), (36, 36)):
        out.append(G(2, 128, H, W, 72, 4, stride=2, pad=1, transposed=1))
        out.append(G(1, 64, H, W, 1024, (4, 1), stride=(2, 1), pad=(1, 0), transposed=1))
        out.append(G(1, 64, H, W, 72, 3, stride=1, pad=1, transposed=1))
        out.append(G(1, 64, H, W, 72, 2, stride=2, transposed=1))
    return out


def _patch():
    """conv3x3p_plan: 199 / 200 tiles, waste 1.13 in both axes, Cin 448 / 512 (split), min_cin 128 / 256, the adjoint's
    width and height rules, pad 0 .. 3, the three padding modes."""
    out = []
    shapes = ((1, 397, 64), (1, 399, 64), (1, 400, 64), (1, 50, 250), (1, 49, 250), (1, 50, 226), (1, 50, 227),
              (25, 7, 64), (25, 9, 64), (2, 24, 192), (2, 23, 192), (1, 50, 128), (1, 50, 120), (4, 50, 128))
    for pm in (0, 1, 2):
        for Cin in (128, 192, 256, 512):
            for Cout in (64, 128, 192):
                for N, H, W in shapes:
                    out.append(G(N, Cin, H, W, Cout, 3, pad=1, pad_mode=pm))
    # the split forms: variant 4 (4 rows), 3 (2 rows), Hin % 4 for the adjoint, kch / 2 >= 2, 199 / 200 workgroups
    for pm in (0, 1, 2):
        for Cin in (128, 448, 512, 1024):
            for Cout in (64, 768, 1024):
                for N, H, W in ((3, 9, 64), (3, 10, 64), (3, 11, 64), (3, 12, 64), (1, 32, 64)):
                    out.append(G(N, Cin, H, W, Cout, 3, pad=1, pad_mode=pm))
    for pad in (0, 2, 3):
        for pm in (0, 1):
            for N, H, W, Cin, Cout in ((2, 25, 192, 256, 192), (1, 51, 122, 256, 1024), (3, 13, 66, 512, 768), (1, 3, 3, 256, 64)):
                out.append(G(N, Cin, H, W, Cout, 3, pad=pad, pad_mode=pm))
    out.append(G(2, 256, 23, 190, 192, 3, pad=(1, 2)))
    out.append(G(2, 256, 23, 190, 192, 3, pad=1, out_f32=1))
    out.append(G(2, 256, 46, 380, 192, 3, stride=2, pad=1))
    return out


def _special():
    """conv1x7_thin_plan, conv7x1_col_plan and conv_dot_ok: each condition on both sides."""
    out = []
    for Cin in (64, 128, 192):
        for Cout in (1, 4, 32, 33):
            for W in (3, 4, 129):
                for f32, act in ((1, 0), (0, 0), (1, 1)):
                    out.append(G(2, Cin, 3, W, Cout, (1, 7), pad=(0, 3), pad_mode=1, out_f32=f32, act=act, ldy=(Cout + 3) & ~3))
    out.append(G(2, 64, 3, 9, 4, (1, 7), pad=(0, 3), pad_mode=0, out_f32=1))
    out.append(G(2, 64, 3, 9, 4, (1, 7), pad=(0, 2), pad_mode=1, out_f32=1))
    out.append(G(2, 64, 3, 9, 3, (1, 7), pad=(0, 3), pad_mode=1, out_f32=1))           # ldy % 4 != 0
    for Cin in (64, 128):
        for Cout in (64, 128, 192):
            for H in (3, 4, 9):
                for pm, act in ((1, 0), (0, 0), (1, 1)):
                    out.append(G(2, Cin, H, 33, Cout, (7, 1), pad=(3, 0), pad_mode=pm, act=act))
    out.append(G(2, 64, 9, 33, 64, (7, 1), pad=(3, 0), pad_mode=1, out_f32=1))
    out.append(G(2, 64, 9, 33, 64, (7, 1), stride=(2, 1), pad=(3, 0), pad_mode=1))
    for Cin in (448, 512, 576, 1024):
        for Cout in (1, 2):
            for k, pad in ((1, 0), (4, 1), ((3, 5), 1), ((1, 17), 0)):
                for f32 in (0, 1):
                    out.append(G(1, Cin, 6, 20, Cout, k, pad=pad, out_f32=f32))
    for kw in (dict(pad=1, pad_mode=1), dict(transposed=1), dict(ldx=520, ci_off=8), dict(ldx=520, ci_off=4), dict(ldx=516)):
        out.append(G(2, 512, 5, 7, 1, 3, out_f32=1, **kw))
    return out


def _views():
    """Channel-slice views and stats_per_sample on every kind of kernel."""
    out = []
    bases = (dict(a=(2, 64, 5, 7, 72, 3), k=dict(pad=1)),                                        # implicit GEMM
             dict(a=(2, 64, 5, 7, 3, 3), k=dict(pad=1)),                                         # ... Cout % 4 != 0
             dict(a=(2, 256, 23, 190, 192, 3), k=dict(pad=1, pad_mode=1)),                       # patch
             dict(a=(2, 64, 9, 33, 128, (7, 1)), k=dict(pad=(3, 0), pad_mode=1)),                # column
             dict(a=(2, 64, 3, 9, 4, (1, 7)), k=dict(pad=(0, 3), pad_mode=1, out_f32=1)),        # thin
             dict(a=(2, 64, 5, 7, 72, 3), k=dict(pad=1, transposed=1, stride=2)))                # classes
    for b in bases:
        Cin, Cout = b["a"][1], b["a"][4]
        views = [dict(ldx=Cin + 8, ci_off=8), dict(ldx=Cin + 64, ci_off=0), dict(ldx=Cin + 8, ci_off=4), dict(ldx=Cin + 4),
                 dict(ldx=Cin + 8, ci_off=16), dict(ci_off=-8, ldx=Cin + 8), dict(ldy=Cout + 8, co_off=8),
                 dict(ldy=Cout + 8, co_off=4), dict(ldy=Cout + 4, co_off=4), dict(ldy=Cout + 2, co_off=1), dict(ldy=Cout + 8, co_off=9),
                 dict(ldy=Cout + 8, co_off=-1), dict(ldy=Cout - 1), dict(sps=1), dict(sps=1, ldy=Cout + 8, co_off=8)]
        for v in views:
            out.append(G(*b["a"], **b["k"], **v))
    for N in (1, 3):
        out.append(G(N, 64, 25, 53, 1024, 1, sps=1))
        out.append(G(N, 512, 6, 20, 1, 4, pad=1, out_f32=1, sps=1))
    return out


def _wgrad():
    """plan9's Win % 64, plan_line's tl <= 2 || tl >= 128 and its kernel shapes, the one-tap cost model's split count."""
    out = []
    for W in (63, 64, 65, 128, 192):
        for H in (1, 2, 3, 17):
            for Cin, Cout in ((64, 64), (128, 192), (72, 64), (64, 8)):
                out.append(G(2, Cin, H, W, Cout, 3, pad=1, pad_mode=H % 2))
    out.append(G(1, 64, 4, 64, 64, 3, pad=0))
    out.append(G(1, 64, 9, 128, 64, 3, stride=2, pad=1))
    for Cin, Cout in ((64, 64), (64, 128), (64, 192), (128, 128), (512, 512), (448, 1024), (512, 1024), (1024, 1024), (72, 64)):
        for tr in (0, 1):
            for pm in (0, 1):
                if not (tr and pm):
                    out.append(G(1, Cin, 9, 11, Cout, 3, stride=2, pad=1, pad_mode=pm, transposed=tr, output_padding=tr))
    for k, pad in (((7, 1), (3, 0)), ((1, 7), (0, 3)), ((4, 1), (1, 0)), ((7, 1), (3, 1)), ((4, 1), (1, 1)), ((5, 1), (2, 0))):
        for stride in (1, (2, 1), (1, 2)):
            for H, W in ((9, 70), (19, 5), (130, 200)):
                for Cin, Cout in ((64, 64), (128, 64), (72, 64)):
                    out.append(G(1, Cin, H, W, Cout, k, stride=stride, pad=pad, pad_mode=int(Cin == 128)))
    out.append(G(1, 64, 3, 5, 64, (7, 1), pad=(3, 0), pad_mode=1))                  # reflect pad >= extent
    out.append(G(1, 64, 9, 70, 64, (7, 1), pad=(3, 0), transposed=1))
    for Cin, Cout in ((8, 8), (64, 72), (72, 24), (200, 136), (1024, 1024)):
        for k, stride, pad in ((1, 1, 0), (3, 1, 1), (4, 2, 1), (7, 1, 3)):
            for N, H, W in ((1, 5, 7), (1, 16, 16), (2, 33, 31), (1, 64, 64), (1, 128, 128), (2, 256, 256)):
                if Cin * Cout * N * H * W <= 1 << 34:
                    out.append(G(N, Cin, H, W, Cout, k, stride=stride, pad=pad))
    return out


def _invalid():
    """One descriptor (or more) per error return of make_plan, plan and the special plans."""
    ok = G(2, 64, 9, 11, 72, 3, pad=1)
    tr = G(2, 64, 5, 7, 72, 3, stride=2, pad=1, transposed=1)
    out = [dict(ok, Cin=48), dict(ok, Cin=32), dict(ok, Cin=0), dict(ok, Cin=100), dict(ok, Hout=ok["Hout"] + 1),
           dict(ok, Wout=ok["Wout"] - 1), dict(ok, dtype=7), dict(ok, dtype=0), dict(ok, pad_mode=3), dict(ok, pad_mode=2),
           dict(ok, pad_mode=-1), dict(ok, N=0), dict(ok, Cout=0), dict(ok, Cout=4), dict(ok, stride_h=0), dict(ok, pad_w=-1),
           dict(ok, kh=0), G(1, 64, 9, 11, 72, (8, 7), pad=3), dict(tr, stride_h=3, Hout=tr["Hout"] + 4), dict(tr, pad_mode=1),
           dict(tr, Hout=tr["Hout"] - 1), dict(tr, Wout=tr["Wout"] + 2), dict(tr, stats_per_sample=1),
           G(1, 64, 5, 7, 72, 1, stride=2, transposed=1),                               # a class without taps
           G(1, 64, 3, 9, 72, 7, pad=3, pad_mode=1), G(1, 64, 9, 2, 72, 5, pad=2, pad_mode=1),  # reflect pad >= extent
           G(32768, 64, 256, 256, 64, 1), G(1, 64, 4096, 4096, 64, 1), G(1, 64, 2, 2, 64, 1, ldx=1 << 29),
           G(1, 16384, 2, 2, 16384, 3, pad=1), G(1, 64, 2048, 2048, 512, 3, pad=1),     # pixels, X bytes, W bytes, Y bytes
           G(4, 256, 1024, 1024, 256, 3, pad=1, pad_mode=1), G(1, 64, 2048, 4096, 64, (7, 1), pad=(3, 0), pad_mode=1),
           G(8, 64, 1024, 4096, 4, (1, 7), pad=(0, 3), pad_mode=1, out_f32=1)]
    return out


def descriptors():
    """The fixed list, as tuples in the order of DESC_FIELDS, without repeats."""
    both = _recorded()
    grid = _tile_pixels() + _classes() + _patch() + _special() + _views() + _wgrad() + _invalid()
    out, seen = [], set()
    for d, dtypes in [(d, (BF16, F16)) for d in both] + [(d, (d["dtype"],)) for d in grid]:
        for dt in dtypes:
            t = tuple(int(dict(d, dtype=dt)[f]) for f in DESC_FIELDS)
            if t not in seen:
                seen.add(t)
                out.append(t)
    # the grid in the second element type: every tenth descriptor
    for d in grid[::10]:
        t = tuple(int(dict(d, dtype=F16)[f]) for f in DESC_FIELDS)
        if t not in seen and d["dtype"] == BF16:
            seen.add(t)
            out.append(t)
    return out


def _pack(lib, _lib, desc):
    rec = []
    for adjoint, off in PACK_JOBS:
        job = _lib.PackJob(desc, W_PTR + off, WP_PTR, adjoint, 0)
        need = lib.ir2rgb_conv2d_pack_batch_table_bytes(ctypes.byref(job), 1)
        if need < 0:
            rec.append(need)
            continue
        table = (ctypes.c_char * need)()
        nblocks = ctypes.c_int(-1)
        n = lib.ir2rgb_conv2d_pack_batch_build(ctypes.byref(job), 1, ctypes.cast(table, ctypes.c_void_p), need, ctypes.byref(nblocks))
        rec.append([need, n, nblocks.value, hashlib.sha1(bytes(table)).hexdigest()])
    return rec


def answers(lib, descs):
    """-> (rows, pack records) of the built library for the descriptor tuples."""
    from ir2rgb_amd import _lib
    rows, packs, index = [], [], {}
    for t in descs:
        desc = _lib.ConvDesc(*t)
        p = ctypes.byref(desc)
        pack = _pack(lib, _lib, desc)
        key = json.dumps(pack)
        if key not in index:
            index[key] = len(packs)
            packs.append(pack)
        # The seventh column calls a launch entry point, with arguments it must refuse before it touches a stream: x
        # misaligned, dw and workspace NULL (wgrad_impl checks both right after the descriptor).  Were that check lost,
        # the NULL dw would still be refused by the row comparison, but only after a launch on a machine with a GPU.
        rows.append([NAMES.index(lib.ir2rgb_conv2d_kernel_name(p).decode()), lib.ir2rgb_conv2d_stats_rows(p),
                     lib.ir2rgb_conv2d_packed_weight_elems(p), lib.ir2rgb_conv2d_fwd_workspace_bytes(p),
                     lib.ir2rgb_conv2d_wgrad_workspace_elems(p), lib.ir2rgb_conv2d_wgrad_acc_workspace_elems(p),
                     lib.ir2rgb_conv2d_wgrad(p, 8, 16, None, None, None), index[key]])
    return rows, packs


def main():
    from ir2rgb_amd import _lib
    for v in ("IR2RGB_CONV3X3P", "IR2RGB_CONV3X3P_SPLIT", "IR2RGB_CONV_DOT"):
        assert v not in os.environ, v
    descs = descriptors()
    rows, packs = answers(_lib.lib(), descs)
    listing = hashlib.sha1(json.dumps(descs).encode()).hexdigest()
    with open(PATH, "w") as f:
        f.write('{"names": %s,\n "descriptors": %d, "descriptors_sha1": "%s",\n "pack": [\n' % (json.dumps(NAMES), len(descs), listing))
        f.write(",\n".join(json.dumps(p, separators=(",", ":")) for p in packs))
        f.write('],\n "rows": [\n')
        f.write(",\n".join(json.dumps(r, separators=(",", ":")) for r in rows))
        f.write("]}\n")
    print(len(descs), "descriptors,", len(packs), "pack records,", os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    main()
