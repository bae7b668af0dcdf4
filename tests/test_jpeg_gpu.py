"""JPEG encoding on the GPU (ir2rgb_amd.jpeg.JpegEncoder, csrc/jpeg.hip).  Every step runs in a child process of its own
under its own time limit (``python tests/test_jpeg_gpu.py <step>``), as in tests/test_scale_gpu.py.  Every comparison is
equality: the kernels do integer arithmetic.  The steps read only tests/golden/jpeg_cases.npz (files recorded from Pillow)
and ``jpeg.jpeg_reference``; neither Pillow nor the reference is needed, but for the host half of ``snapshots``, where
Pillow is what ``Snapshots(encoder="host")`` itself calls.

  kernels     every golden case (three modes, five qualities, restart_rows 1 and 2, ten shapes, the extras: saturated
              checkerboards, a flat frame, sparse pixels, intervals longer than one chunk of the entropy kernel), mode L from
              C = 1 and C = 3 frames: bytes and length, canary bands around the output and the workspace, bytes past the
              length untouched; three frames in one call against three calls; a source misaligned by one byte; the error
              codes before any launch
  fullsize    one 512x1024 frame per mode: SHA-256 and length of Pillow's file
  translator  five frames through VideoTranslator.save at 64x128 against jpeg_reference of the frames translate yields,
              use_graph on and off, other options; submit / collect ordering across two submissions
  snapshots   Snapshots(encoder="device") against jpeg_reference of the composed stack (mode L for one-channel panels);
              encoder="host" writes what write_images writes
"""
import copy
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
G_OPT = dict(gen_blocks=9, n_blocks_local=3, fg=False, no_flow=False, n_local_enhancers=1, feat_num=3)
TG = 3
GUARD = 32768


def _run(step, seconds):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), step], capture_output=True, text=True, timeout=seconds,
                       cwd=ROOT)
    print(r.stdout[-6000:])
    assert r.returncode == 0, f"step {step} ended with {r.returncode}:\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    assert f"step {step} ok" in r.stdout


def test_jpeg_kernels_equal_pillow(dev):
    _run("kernels", 300)


def test_full_size_frames_equal_pillow(dev):
    _run("fullsize", 120)


def test_translator_saves_the_frames_it_yields(dev):
    _run("translator", 300)


def test_snapshots_encode_on_the_device(dev):
    _run("snapshots", 120)


# =============================================================================================
# the steps (child process)
# =============================================================================================
class Guarded:
    """``n`` bytes inside a larger allocation whose neighbourhood holds a canary; ``skew`` shifts the start."""

    def __init__(self, shape, dev, fill, junk, skew=0, dtype=torch.uint8):
        n = int(np.prod(shape))
        self.fill = fill
        self.buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev)
        self.t = self.buf[GUARD + skew:GUARD + skew + n].view(shape)
        self.t.fill_(junk)
        self.lo, self.hi = GUARD + skew, GUARD + skew + n

    def intact(self):
        return bool((self.buf[:self.lo] == self.fill).all() and (self.buf[self.hi:] == self.fill).all())


def _goldens():
    import make_jpeg_goldens as G
    d = np.load(G.PATH)
    cases = json.loads(str(d["cases"]))
    files = d["files"]
    return [(m, d[m["src"]], files[m["offset"]:m["offset"] + m["length"]].tobytes()) for m in cases], json.loads(str(d["fullsize"]))


_ENCODERS = {}


def _encoder(dev, h, w, c, m):
    from ir2rgb_amd.jpeg import JpegEncoder
    key = (h, w, c, m["quality"], m["mode"], m["restart_rows"])
    if key not in _ENCODERS:
        _ENCODERS[key] = JpegEncoder(dev, h, w, channels=c, quality=m["quality"], subsampling=m["mode"], restart_rows=m["restart_rows"])
    return _ENCODERS[key]


def _encode_checked(enc, frames, what, src_skew=0):
    """One call with canaries around the output and the workspace -> the files; the bytes past each length are untouched."""
    n = frames.shape[0]
    src = Guarded(tuple(frames.shape), frames.device, 0x11, 0, skew=src_skew)
    src.t.copy_(frames)
    out = Guarded((n, enc.capacity), frames.device, 0xA5, 0x3C)
    ws = Guarded((enc.workspace_bytes(n),), frames.device, 0x5A, 0xC3)
    lengths = Guarded((n,), frames.device, -7, -1, dtype=torch.int32)
    enc.encode_into(src.t, out.t, lengths.t, ws.t)
    torch.cuda.synchronize()
    assert out.intact(), f"{what}: wrote outside the output"
    assert ws.intact(), f"{what}: wrote outside the workspace"
    assert lengths.intact() and src.intact() and torch.equal(src.t, frames), what
    got, host = [], out.t.cpu()
    for i, m in enumerate(lengths.t.cpu().tolist()):
        assert len(enc.header) < m <= enc.capacity, f"{what}: length {m}"
        assert bool((host[i, m:] == 0x3C).all()), f"{what}: bytes past the length were written"
        got.append(host[i, :m].numpy().tobytes())
    return got


def step_kernels(dev):
    from ir2rgb_amd import _lib
    from ir2rgb_amd.jpeg import JpegEncoder, jpeg_reference
    cases, _ = _goldens()
    names = {m["name"].split("/")[0] for m, _, _ in cases}
    assert {"checker", "checker_odd", "flat", "sparse", "long_interval", "1x1", "144x40", "17x33"} <= names and len(cases) == 330
    on_device = {}
    for m, src, want in cases:
        h, w = m["hw"]
        if m["src"] not in on_device:
            on_device[m["src"]] = torch.from_numpy(src).to(dev).unsqueeze(0)
        frames = on_device[m["src"]]
        forms = [(3, frames)]
        if m["mode"] == "L":
            forms.append((1, frames[..., :1].contiguous()))
        for c, f in forms:
            got = _encode_checked(_encoder(dev, h, w, c, m), f, f"{m['name']} C={c}")
            assert got == [want], f"{m['name']} C={c}: {len(got[0])} bytes, {len(want)} expected"
    print(f"kernels: {len(cases)} golden cases exact (mode L from C = 1 and 3), canaries intact")
    # a source off the dword boundary by one byte
    for name in ("17x33/4:2:0/q75/r1", "31x47/4:4:4/q95/r2", "13x21/L/q30/r1"):
        m, src, want = next(c for c in cases if c[0]["name"] == name)
        got = _encode_checked(_encoder(dev, *m["hw"], 3, m), on_device[m["src"]], name + " misaligned source", src_skew=1)
        assert got == [want], name
    print("kernels: source misaligned by one byte exact")
    # three frames in one call = three calls = Pillow
    for mode in ("4:2:0", "4:4:4", "L"):
        trio = [next(c for c in cases if c[0]["name"] == f"{n}/{mode}/{q}/r1") for n, q in (("17x33", "q75"), ("flat", "q75"),
                                                                                          ("17x33", "q75"))]
        batch = torch.cat([on_device[m["src"]] for m, _, _ in trio])
        batch[2] = batch[2].flip(1)                                     # a third, different frame
        enc = _encoder(dev, 17, 33, 3, trio[0][0])
        got = _encode_checked(enc, batch, f"batch of 3 {mode}")
        assert got[:2] == [trio[0][2], trio[1][2]] and got == jpeg_reference(batch, 75, mode, 1)
        assert got == [_encode_checked(enc, batch[i:i + 1], f"one of 3 {mode}")[0] for i in range(3)]
        assert enc.encode(batch) == got and enc.encode(batch[1]) == got[1:2]
    print("kernels: one call of three frames = three calls")
    # refused before any launch: nothing is written
    m, src, want = next(c for c in cases if c[0]["name"] == "17x33/4:2:0/q75/r1")
    enc = _encoder(dev, 17, 33, 3, m)
    f = on_device[m["src"]]
    out = Guarded((1, enc.capacity), dev, 0xA5, 0x3C)
    ws = Guarded((enc.workspace_bytes(1),), dev, 0x5A, 0xC3)
    lengths = torch.full((4,), -1, dtype=torch.int32, device=dev)
    lib = _lib.lib()

    def call(src=f, out_=out.t, lengths_=lengths, ws_=ws.t, ws_bytes=None, header=enc._header, header_bytes=len(enc.header),
             tables=enc._tables, N=1, C=3, H=17, W=33, mode=1, rr=1, capacity=enc.capacity):
        p = [None if t is None else (t if isinstance(t, int) else t.data_ptr()) for t in (src, out_, lengths_, ws_, header, tables)]
        return lib.ir2rgb_jpeg_encode_u8(p[0], p[1], p[2], p[3], ws.t.numel() if ws_bytes is None else ws_bytes, p[4], header_bytes,
                                         p[5], N, C, H, W, mode, rr, enc.max_dc, enc.max_ac, capacity, None)

    for kw in (dict(src=None), dict(out_=None), dict(lengths_=None), dict(ws_=None), dict(header=None), dict(tables=None),
               dict(ws_bytes=ws.t.numel() - 1), dict(capacity=enc.capacity - 1), dict(rr=0), dict(N=0), dict(C=1), dict(C=4),
               dict(mode=-1), dict(mode=3), dict(H=0), dict(W=70000), dict(header_bytes=0)):
        assert call(**kw) == -1, kw
    for kw in (dict(ws_=ws.t.data_ptr() + 4), dict(tables=enc._tables.data_ptr() + 2), dict(lengths_=lengths.data_ptr() + 2)):
        assert call(**kw) == -3, kw
    torch.cuda.synchronize()
    assert out.intact() and ws.intact() and bool((out.t == 0x3C).all()) and bool((ws.t == 0xC3).all()) and bool((lengths == -1).all())
    for bad in (dict(restart_rows=0), dict(subsampling="4:2:2"), dict(channels=1), dict(channels=2)):
        with pytest.raises(ValueError):
            JpegEncoder(dev, 17, 33, **bad)
    with pytest.raises(ValueError):
        enc.encode(f[:, :-1].contiguous())
    with pytest.raises(ValueError):
        enc.encode(f.cpu())
    with pytest.raises(TypeError):
        enc.encode(f.float())
    print("kernels: bad arguments refused before any launch")


def step_fullsize(dev):
    import make_jpeg_goldens as G
    from ir2rgb_amd.jpeg import JpegEncoder
    _, full = _goldens()
    frame = torch.from_numpy(G.fullsize_frame()).to(dev).unsqueeze(0)
    assert [f["mode"] for f in full] == ["4:4:4", "4:2:0", "L"]
    for f in full:
        enc = JpegEncoder(dev, 512, 1024, quality=f["quality"], subsampling=f["mode"], restart_rows=f["restart_rows"])
        data, = _encode_checked(enc, frame, f"fullsize {f['mode']}")
        assert len(data) == f["length"] and hashlib.sha256(data).hexdigest() == f["sha256"], f["mode"]
        print(f"fullsize: 512x1024 {f['mode']} exact, {len(data)} bytes of {enc.capacity} reserved")


def _build(ngf, seed):
    from ir2rgb_amd import networks as N
    torch.manual_seed(seed)
    return [N.build_generator_module(3 * TG, 3, 3 * (TG - 1), ngf, "composite", 3, "batch", 0, **G_OPT)]


def _smooth_u8(n, h, w, c, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, c, h, w, generator=g)
    x = torch.tanh(torch.nn.functional.avg_pool2d(torch.nn.functional.pad(x, (2, 2, 2, 2), mode="reflect"), 5, stride=1) * 3)
    return ((x + 1) * 127.5).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def step_translator(dev):
    from ir2rgb_amd.inference import VideoTranslator
    from ir2rgb_amd.jpeg import JpegEncoder, jpeg_reference
    H, W, ngf = 64, 128, 32
    ir = _smooth_u8(5 + TG - 1, H, W, 3, 31).to(dev)
    base = _build(ngf, 33)
    kw = dict(n_scales_spatial=1, first_layer_gen_filters=ngf, first_frame="zeros")
    with tempfile.TemporaryDirectory() as tmp:
        for use_graph in (False, True):
            frames = torch.stack(list(VideoTranslator(dev, H, W, netG=copy.deepcopy(base), use_graph=use_graph, **kw).translate(ir)))
            assert frames.shape == (5, H, W, 3)
            tr = VideoTranslator(dev, H, W, netG=copy.deepcopy(base), use_graph=use_graph, **kw)
            for sub, options in (("default", {}), ("q90", dict(quality=90, subsampling="4:4:4", restart_rows=2))):
                out_dir = os.path.join(tmp, f"{sub}_{int(use_graph)}")
                paths = tr.save(ir, out_dir, **options)
                assert paths == [os.path.join(out_dir, "%06d.jpg" % k) for k in range(5)] and sorted(os.listdir(out_dir)) == \
                    [os.path.basename(p) for p in paths]
                want = jpeg_reference(frames, **options)
                for k, p in enumerate(paths):
                    with open(p, "rb") as f:
                        assert f.read() == want[k], f"graph={use_graph} {sub}: file {k}"
                assert not tr._jpeg[1]._pending
            assert len(tr._graphs) == int(use_graph)
            print(f"translator graph={use_graph}: 5 files = jpeg_reference of the frames translate yields (two option sets)")
    # submit / collect: two submissions in flight come back in order
    enc = JpegEncoder(dev, H, W)
    a, b = frames[:2].contiguous(), frames[2:5].contiguous()
    enc.submit(a)
    enc.submit(b)
    with pytest.raises(RuntimeError):
        enc.submit(a)
    assert enc.collect() == jpeg_reference(a) and enc.collect() == jpeg_reference(b)
    with pytest.raises(RuntimeError):
        enc.collect()
    enc.submit(b[0])
    assert enc.collect() == jpeg_reference(b[:1])
    print("translator: submit / collect keep their order across two submissions")


class _Trainer:
    """What Snapshots.take reads of a trainer."""

    def __init__(self, dev, H, W, seed):
        g = torch.Generator().manual_seed(seed)

        def t(c, scale=1.0):
            return (torch.randn(1, 2, c, H, W, generator=g) * scale).to(dev)
        self.opt = {"input_nc": 1}
        self.last_inputs = (t(1), t(3), t(2, 3.0), t(1).abs().clamp(0, 1))
        self.last_outputs = (t(3), t(3), t(2, 3.0), t(1).abs().clamp(0, 1))
        self.first = t(3)[0, 0]

    def _flow_stream(self, _):
        return None


def step_snapshots(dev):
    from ir2rgb_amd import visuals as V
    from ir2rgb_amd.jpeg import jpeg_reference
    H, W = 64, 128
    trainers = [_Trainer(dev, H, W, 41), _Trainer(dev, H, W, 42)]
    with tempfile.TemporaryDirectory() as tmp:
        device, host = V.Snapshots(dev, os.path.join(tmp, "device"), encoder="device"), V.Snapshots(dev, os.path.join(tmp, "host"))
        assert host.encoder == "host"
        for epoch, tr in enumerate(trainers, 1):
            device.take(tr, epoch, tr.first)
            host.take(tr, epoch, tr.first)
        device.flush(), host.flush()
        assert host._jpeg is None and device._host == [None, None]
        for epoch, tr in enumerate(trainers, 1):
            plist = V.panels(V.trainer_tensors(tr, tr.first), tr.opt)
            stack = V.compose(plist).cpu()
            assert [t.shape[0] for _, _, t in plist] == [1, 3, 3, 3, 3, 2, 1, 2, 1]
            V.write_images(os.path.join(tmp, "parent"), epoch, [(n, t.shape[0]) for n, _, t in plist], stack.numpy())
            for i, (name, _, t) in enumerate(plist):
                grey = t.shape[0] == 1
                file = V.image_name(epoch, name, "jpg")
                with open(os.path.join(tmp, "device", "images", file), "rb") as f:
                    assert f.read() == jpeg_reference(stack[i:i + 1], 75, "L" if grey else "4:2:0", 1)[0], (epoch, name)
                with open(os.path.join(tmp, "host", "images", file), "rb") as f:
                    got = f.read()
                with open(os.path.join(tmp, "parent", file), "rb") as f:
                    assert got == f.read(), (epoch, name)
                assert got == jpeg_reference(stack[i:i + 1], 75, "L" if grey else "4:2:0", 0)[0], (epoch, name)
        assert os.path.exists(os.path.join(tmp, "device", "index.html"))
    with pytest.raises(ValueError):
        V.Snapshots(dev, "x", fmt="png", encoder="device")
    with pytest.raises(ValueError):
        V.Snapshots(dev, "x", encoder="gpu")
    print("snapshots: device files = jpeg_reference of the stack (L for one channel); host files = write_images")


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    step = sys.argv[1]
    assert torch.cuda.is_available()
    globals()["step_" + step](torch.device("cuda:0"))
    torch.cuda.synchronize()
    print(f"step {step} ok", flush=True)
