"""JPEG decoding on the GPU (ir2rgb_amd.jpeg_decode.JpegDecoder, csrc/jpeg_decode.hip).  Every step runs in a child process
of its own under its own time limit (``python tests/test_jpeg_decode_gpu.py <step>``), as in tests/test_jpeg_gpu.py.  Every
comparison is equality: the kernels do integer arithmetic.  The steps read only tests/golden/jpeg_decode_cases.npz (files
written and decoded by Pillow), ``jpeg_decode.decode_reference`` and ``jpeg.jpeg_reference``; Pillow is not needed.

  kernels       every golden case: pixels and status 0, canary bands around output, workspace, status and the uploaded
                block (which stays as it was); three files with different tables and restart intervals in one call against
                three calls; scan bytes off the dword boundary by one byte; mode L into three channels; the error codes
                before any launch
  subsequences  every golden case at forced sub_bytes 4, 16 and 64: the pixels of the default
  malformed     a scan truncated mid-block, one flipped byte, a segment record with one MCU too many: the call returns, the
                status is the one jpeg_decode.entropy_model gives, canaries intact, decode() raises ValueError
  fullsize      one 512x640 file per mode without restart markers: SHA-256 of Pillow's pixels
  roundtrip     JpegEncoder's files at 64x128 decode to decode_reference of the same bytes; submit / collect ordering
  pipeline      tr.save(dec.frames(files), dir) writes the files tr.save writes from host-decoded frames;
                FolderSequences.sequence() = scaled_sequence on decode_reference frames, bit for bit; two epochs of fit
"""
import copy
import hashlib
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
GUARD = 32768


def _run(step, seconds):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), step], capture_output=True, text=True, timeout=seconds,
                       cwd=ROOT)
    print(r.stdout[-6000:])
    assert r.returncode == 0, f"step {step} ended with {r.returncode}:\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    assert f"step {step} ok" in r.stdout


def test_jpeg_decode_kernels_equal_pillow(dev):
    _run("kernels", 300)


def test_pixels_do_not_depend_on_the_subsequence_size(dev):
    _run("subsequences", 300)


def test_malformed_files_are_reported_not_trusted(dev):
    _run("malformed", 120)


def test_full_size_files_equal_pillow(dev):
    _run("fullsize", 120)


def test_decoder_reads_what_the_encoder_writes(dev):
    _run("roundtrip", 120)


def test_files_to_files_and_files_to_fit(dev):
    _run("pipeline", 300)


# =============================================================================================
# the steps (child process)
# =============================================================================================
class Guarded:
    """``n`` elements inside a larger allocation whose neighbourhood holds a canary."""

    def __init__(self, shape, dev, fill, junk, dtype=torch.uint8):
        n = int(np.prod(shape))
        self.fill = fill
        self.buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev)
        self.t = self.buf[GUARD:GUARD + n].view(shape)
        self.t.fill_(junk)
        self.lo, self.hi = GUARD, GUARD + n

    def intact(self):
        return bool((self.buf[:self.lo] == self.fill).all() and (self.buf[self.hi:] == self.fill).all())


_DECODERS = {}


def _decoder(dev, h, w, mode, c=None):
    from ir2rgb_amd.jpeg_decode import JpegDecoder
    key = (h, w, mode, c)
    if key not in _DECODERS:
        _DECODERS[key] = JpegDecoder(dev, h, w, mode, channels=c)
    return _DECODERS[key]


def _decode_checked(dec, infos, what, sub_bytes=None, skew=0):
    """One call with canaries around everything it is given -> (pixels uint8 [N,H,W,C] numpy, status list)."""
    dev, n = dec.device, len(infos)
    block, n_seg, layout = dec.pack(infos, skew=skew)
    staged = Guarded((block.size,), dev, 0x11, 0)
    staged.t.copy_(torch.from_numpy(block))
    out = Guarded((n, dec.H, dec.W, dec.C), dev, 0xA5, 0x3C)
    ws = Guarded((dec.workspace_bytes(n, n_seg),), dev, 0x5A, 0xC3)
    status = Guarded((n,), dev, -7, -1, dtype=torch.int32)
    dec.decode_into(staged.t, n, n_seg, layout, out.t, status.t, ws.t, sub_bytes)
    torch.cuda.synchronize()
    assert out.intact(), f"{what}: wrote outside the output"
    assert ws.intact(), f"{what}: wrote outside the workspace"
    assert status.intact(), f"{what}: wrote outside the status"
    assert staged.intact() and np.array_equal(staged.t.cpu().numpy(), block), f"{what}: the uploaded files changed"
    return out.t.cpu().numpy(), status.t.cpu().tolist()


def _goldens():
    import make_jpeg_decode_goldens as G
    from ir2rgb_amd.jpeg_decode import parse
    cases, full = G.load()
    return [(m, parse(data), want) for m, data, want in cases], full


def _shaped(want, c):
    """Pillow's array as the decoder's [H,W,C]"""
    if want.ndim == 2:
        want = want[..., None]
    return np.repeat(want, c, axis=2) if want.shape[2] != c else want


def step_kernels(dev):
    from ir2rgb_amd import _lib
    from ir2rgb_amd.jpeg_decode import JpegDecoder, TABLE_WORDS
    cases, _ = _goldens()
    assert len(cases) == 196
    for m, info, want in cases:
        dec = _decoder(dev, *m["hw"], m["mode"])
        got, status = _decode_checked(dec, [info], m["name"])
        assert status == [0], f"{m['name']}: status {status}"
        assert np.array_equal(got[0], _shaped(want, dec.C)), f"{m['name']}: pixels differ"
    print(f"kernels: {len(cases)} golden cases exact, status 0, canaries intact")
    by_name = {m["name"]: (m, info, want) for m, info, want in cases}
    # mode L into three channels: Image.convert("RGB")
    m, info, want = by_name["17x33/L/q75"]
    got, status = _decode_checked(_decoder(dev, 17, 33, "L", 3), [info], "L into RGB")
    assert status == [0] and np.array_equal(got[0], _shaped(want, 3))
    # scan bytes off the dword boundary by one byte
    for name in ("17x33/4:2:0/q75", "31x47/4:4:4/q95", "9x17/4:2:2/q30", "64x80/L/q100"):
        m, info, want = by_name[name]
        dec = _decoder(dev, *m["hw"], m["mode"])
        got, status = _decode_checked(dec, [info], name + " misaligned", skew=1)
        assert status == [0] and np.array_equal(got[0], _shaped(want, dec.C)), name
    print("kernels: scan bytes misaligned by one byte exact")
    # three files with different tables and restart intervals in one call = three calls = Pillow
    for mode in ("4:2:0", "4:4:4", "4:2:2", "L"):
        trio = [by_name[f"64x80/{mode}/q{q}"] for q in (1, 75, 100)]
        assert len({(m["restart_rows"], m["optimize"]) for m, _, _ in trio}) > 1
        dec = _decoder(dev, 64, 80, mode)
        got, status = _decode_checked(dec, [info for _, info, _ in trio], f"batch of 3 {mode}")
        assert status == [0, 0, 0]
        for i, (m, info, want) in enumerate(trio):
            assert np.array_equal(got[i], _shaped(want, dec.C)), (mode, i)
            assert np.array_equal(_decode_checked(dec, [info], f"one of 3 {mode}")[0][0], got[i])
        assert np.array_equal(dec.decode([info.data for _, info, _ in trio]).cpu().numpy(), got)
    print("kernels: one call of three files = three calls")
    # refused before any launch: nothing is written
    m, info, want = by_name["17x33/4:2:0/q75"]
    dec = _decoder(dev, 17, 33, "4:2:0")
    block, n_seg, (o_tab, o_seg, o_off, o_scan) = dec.pack([info])
    staged = torch.from_numpy(block).to(dev)
    out = Guarded((1, 17, 33, 3), dev, 0xA5, 0x3C)
    ws = Guarded((dec.workspace_bytes(1, n_seg),), dev, 0x5A, 0xC3)
    status = torch.full((4,), -1, dtype=torch.int32, device=dev)
    lib = _lib.lib()
    base = staged.data_ptr()
    assert block.size >= o_tab + 4 * TABLE_WORDS

    def call(files=base + o_scan, offsets=base + o_off, segments=base + o_seg, tables=base + o_tab, out_=out.t.data_ptr(),
             status_=status.data_ptr(), ws_=ws.t.data_ptr(), ws_bytes=ws.t.numel(), N=1, C=3, H=17, W=33, mode=1, n_seg_=n_seg, sub=128):
        return lib.ir2rgb_jpeg_decode_u8(files, offsets, segments, tables, out_, status_, ws_, ws_bytes, N, C, H, W, mode, n_seg_,
                                         sub, None)

    for kw in (dict(files=None), dict(offsets=None), dict(segments=None), dict(tables=None), dict(out_=None), dict(status_=None),
               dict(ws_=None), dict(ws_bytes=ws.t.numel() - 1), dict(N=0), dict(N=70000), dict(C=1), dict(C=4), dict(mode=-1),
               dict(mode=4), dict(H=0), dict(W=70000), dict(n_seg_=0), dict(sub=0)):
        assert call(**kw) == -1, kw
    for kw in (dict(ws_=ws.t.data_ptr() + 4), dict(tables=base + o_tab + 2), dict(segments=base + o_seg + 1),
               dict(offsets=base + o_off + 2), dict(status_=status.data_ptr() + 2)):
        assert call(**kw) == -3, kw
    torch.cuda.synchronize()
    assert out.intact() and ws.intact() and bool((out.t == 0x3C).all()) and bool((ws.t == 0xC3).all()) and bool((status == -1).all())
    assert lib.ir2rgb_jpeg_decode_workspace_bytes(1, 17, 33, 5, 1) == -1
    for bad in (dict(mode="4:1:1"), dict(channels=1), dict(channels=2), dict(sub_bytes=0)):
        with pytest.raises(ValueError):
            JpegDecoder(dev, 17, 33, **{"mode": "4:2:0", **bad})
    with pytest.raises(ValueError, match="17x33"):                       # another geometry: before any launch
        dec.decode([info.data, by_name["9x17/4:2:0/q75"][1].data])
    with pytest.raises(ValueError, match="4:4:4"):
        dec.decode([by_name["17x33/4:4:4/q75"][1].data])
    with pytest.raises(ValueError, match="not a JPEG"):
        dec.decode([b"\x89PNG\r\n\x1a\n" + bytes(32)])
    print("kernels: bad arguments refused before any launch")


def step_subsequences(dev):
    import make_jpeg_decode_goldens as G
    from ir2rgb_amd.jpeg_decode import DEFAULT_SUB_BYTES, ENT_THREADS
    cases, _ = _goldens()
    most = 0
    for m, info, want in cases:
        dec = _decoder(dev, *m["hw"], m["mode"])
        for sub in G.FORCED_SUB_BYTES + (DEFAULT_SUB_BYTES,):
            got, status = _decode_checked(dec, [info], f"{m['name']} sub_bytes {sub}", sub_bytes=sub)
            assert status == [0] and np.array_equal(got[0], _shaped(want, dec.C)), f"{m['name']} sub_bytes {sub}"
            if sub == 4:
                rounds = dec.rounds()
                longest = max(s.end - s.begin for s in info.segments)
                assert int(rounds.max()) <= min(-(-longest // 4), ENT_THREADS)
                most = max(most, int(rounds.max()))
    assert most > 4, "the forced sizes never reach the many-rounds path"
    print(f"subsequences: {len(cases)} cases at sub_bytes {G.FORCED_SUB_BYTES} and the default exact; up to {most} rounds")


def _malformed(cases):
    """[(name, damaged parsed file)]: the inputs tests/test_jpeg_decode_cpu.py runs through entropy_model first."""
    import make_jpeg_decode_goldens as G        # noqa: F401
    from ir2rgb_amd.jpeg_decode import entropy_model, parse
    by_name = {m["name"]: info for m, info, _ in cases}
    out = []
    for name in ("31x47/4:2:0/q75", "64x80/4:4:4/q95", "40x24/L/q100", "17x33/4:2:2/q75"):
        info = by_name[name]
        d = info.data
        a, b = info.scan
        out.append((name + " truncated", parse(d[:a + (b - a) // 2], strict=False)))
        # a flipped byte that lands in value bits leaves a valid stream: take the first position whose damage shows
        for pos in range(a + (b - a) // 3, b):
            if d[pos] in (0xFF, 0x00, 0xAA) or d[pos - 1] == 0xFF:
                continue
            flipped = parse(d[:pos] + bytes([d[pos] ^ 0x55]) + d[pos + 1:], strict=False)
            if any(r["status"] for r in entropy_model(flipped)):
                break
        out.append((name + " flipped", flipped))
        more = parse(d)
        more.segments[-1].n_mcus += 1
        out.append((name + " one MCU too many in the last record", more))
        if len(more.segments) > 1:
            first = parse(d)
            first.segments[0].n_mcus += 1
            out.append((name + " one MCU too many in the first record", first))
    return out


def step_malformed(dev):
    from ir2rgb_amd.jpeg_decode import entropy_model
    cases, _ = _goldens()
    n = 0
    for name, info in _malformed(cases):
        want = 0
        for rec in entropy_model(info):
            want |= rec["status"]
        assert want != 0, name
        dec = _decoder(dev, info.H, info.W, info.mode)
        for sub in (None, 16):
            got, status = _decode_checked(dec, [info], name, sub_bytes=sub)
            assert status == [want], f"{name}: status {status}, the model says {want}"
        with pytest.raises(ValueError, match="damaged JPEG scan"):
            dec.decode([info])
        assert not dec._pending
        n += 1
    print(f"malformed: {n} damaged files return with the model's status, canaries intact, decode() raises")


def step_fullsize(dev):
    import make_jpeg_decode_goldens as G
    from ir2rgb_amd.jpeg_decode import parse
    _, full = _goldens()
    assert [m["mode"] for m, _ in full] == list(G.MODES)
    for m, data in full:
        info = parse(data)
        assert len(info.segments) == 1 and (info.H, info.W) == (512, 640)
        dec = _decoder(dev, 512, 640, m["mode"])
        got, status = _decode_checked(dec, [info], f"fullsize {m['mode']}")
        pixels = got[0][..., 0] if m["mode"] == "L" else got[0]
        assert status == [0] and list(pixels.shape) == m["shape"]
        assert hashlib.sha256(np.ascontiguousarray(pixels).tobytes()).hexdigest() == m["sha256"], m["mode"]
        print(f"fullsize: 512x640 {m['mode']} exact, {len(data)} bytes in one segment, {int(dec.rounds().max())} rounds")


def _smooth_u8(n, h, w, c, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, c, h, w, generator=g)
    x = torch.tanh(torch.nn.functional.avg_pool2d(torch.nn.functional.pad(x, (2, 2, 2, 2), mode="reflect"), 5, stride=1) * 3)
    return ((x + 1) * 127.5).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def step_roundtrip(dev):
    from ir2rgb_amd.jpeg import JpegEncoder
    from ir2rgb_amd.jpeg_decode import JpegDecoder, decode_reference
    H, W = 64, 128
    frames = _smooth_u8(5, H, W, 3, 51).to(dev)
    for mode in ("4:4:4", "4:2:0", "L"):
        files = JpegEncoder(dev, H, W, quality=90, subsampling=mode, restart_rows=2).encode(frames)
        dec = JpegDecoder.for_file(dev, files[0])
        assert (dec.H, dec.W, dec.mode_name) == (H, W, mode)
        got = dec.decode(files).cpu().numpy()
        for i, f in enumerate(files):
            assert np.array_equal(got[i], _shaped(decode_reference(f), dec.C)), (mode, i)
    print("roundtrip: JpegEncoder's files decode to decode_reference of the same bytes (three modes)")
    a, b = files[:2], files[2:5]
    want = [torch.from_numpy(np.stack([_shaped(decode_reference(f), 1) for f in part])) for part in (a, b)]
    dec.submit(a)
    dec.submit(b)
    with pytest.raises(RuntimeError):
        dec.submit(a)
    assert torch.equal(dec.collect().cpu(), want[0]) and torch.equal(dec.collect().cpu(), want[1])
    with pytest.raises(RuntimeError):
        dec.collect()
    assert torch.equal(torch.stack(list(dec.frames(files, chunk=2))).cpu(), torch.cat(want))
    print("roundtrip: submit / collect keep their order across two submissions; frames() in chunks")


def _write_tree(root, n_seq, n_frames, H, W):
    """images/setNN/V000/{lwir,visible}/I%05d.jpg from the repository's own numpy encoder"""
    from ir2rgb_amd.jpeg import jpeg_reference
    for s in range(n_seq):
        ir = _smooth_u8(n_frames, H, W, 1, 70 + s).numpy()
        rgb = _smooth_u8(n_frames, H, W, 3, 80 + s).numpy()
        for track, files in (("lwir", jpeg_reference(ir, 90, "L", 0)), ("visible", jpeg_reference(rgb, 90, "4:2:0", 0))):
            folder = os.path.join(root, "images", "set%02d" % s, "V000", track)
            os.makedirs(folder)
            for k, data in enumerate(files):
                with open(os.path.join(folder, "I%05d.jpg" % k), "wb") as f:
                    f.write(data)


def step_pipeline(dev):
    import random
    from window_stub import stub_flow_and_conf
    from ir2rgb_amd import fit, networks as N, vid2vid as V
    from ir2rgb_amd.frames import FolderSequences, scaled_sequence, video_params
    from ir2rgb_amd.inference import VideoTranslator
    from ir2rgb_amd.jpeg import jpeg_reference
    from ir2rgb_amd.jpeg_decode import JpegDecoder, decode_reference
    from ir2rgb_amd.schedule import TrainingSchedule
    H, W, ngf, TG = 64, 128, 32, 3
    # files -> files: no pixel visits the host
    src = _smooth_u8(5 + TG - 1, H, W, 3, 61).numpy()
    files = jpeg_reference(src, 90, "4:2:0", 0)
    host = torch.from_numpy(np.stack([decode_reference(f) for f in files])).to(dev)
    torch.manual_seed(63)
    g_opt = dict(gen_blocks=9, n_blocks_local=3, fg=False, no_flow=False, n_local_enhancers=1, feat_num=3)
    base = [N.build_generator_module(3 * TG, 3, 3 * (TG - 1), ngf, "composite", 3, "batch", 0, **g_opt)]
    kw = dict(n_scales_spatial=1, first_layer_gen_filters=ngf, first_frame="zeros")
    with tempfile.TemporaryDirectory() as tmp:
        paths = [os.path.join(tmp, "in_%02d.jpg" % k) for k in range(len(files))]
        for p, data in zip(paths, files):
            with open(p, "wb") as f:
                f.write(data)
        dec = JpegDecoder.for_file(dev, paths[0])
        a = VideoTranslator(dev, H, W, netG=copy.deepcopy(base), **kw).save(dec.frames(paths, chunk=3), os.path.join(tmp, "device"))
        b = VideoTranslator(dev, H, W, netG=copy.deepcopy(base), **kw).save(host, os.path.join(tmp, "host"))
        assert len(a) == len(b) == 5
        for pa, pb in zip(a, b):
            with open(pa, "rb") as fa, open(pb, "rb") as fb:
                assert fa.read() == fb.read(), pa
        print("pipeline: save(dec.frames(paths)) writes the 5 files save() writes from host-decoded frames")
        # files -> fit
        root = os.path.join(tmp, "data")
        _write_tree(root, 2, 6, H, W)
        opt = dict(dataset_scale="resize", dataset_crop="none", load_size=128, fine_size=128, is_train=True, flip=True,
                   n_input_gen_frames=TG, max_frames_per_gpu=1, max_t_step=2)
        seqs = FolderSequences(dev, os.path.join(root, "images"), rng=(random.Random(7), np.random.RandomState(7)), **opt)
        assert len(seqs) == 2 and seqs.seq_len_max == 6
        ir, rgb = seqs.sequence(1, 2)
        index, n, start, step, scaler = seqs.last
        assert (n, start, step) == video_params(6, 1, rng=np.random.RandomState(7), n_frames_total=2, **opt) and n == 4
        picked = [start + i * step for i in range(n)]
        ref = [torch.from_numpy(np.stack([_shaped(decode_reference(open(track[1][i], "rb").read()), 3) for i in picked])).to(dev)
               for track in (seqs.ir_paths, seqs.rgb_paths)]
        wa, wb, _ = scaled_sequence(ref[0], ref[1], scaler=scaler)
        assert ir.shape == (1, n, 3, *scaler.out_hw) and torch.equal(ir.reshape(wa.shape), wa) and torch.equal(rgb.reshape(wb.shape), wb)
        print("pipeline: FolderSequences.sequence() = scaled_sequence on decode_reference frames, bit for bit")
    with tempfile.TemporaryDirectory() as tmp:
        _write_tree(tmp, 2, 6, H, W)
        opt = dict(dataset_scale="none", dataset_crop="none", n_input_gen_frames=TG, max_frames_per_gpu=1, max_t_step=1)
        seqs = FolderSequences(dev, os.path.join(tmp, "images"), rng=(random.Random(9), np.random.RandomState(9)), **opt)
        tr = V.Vid2VidTrainer(dev, compute_dtype=torch.bfloat16, n_scales_spatial=2, build_flow_net=False,
                              first_layer_gen_filters=32, niter_fix_global=1)
        tr.flow_net = stub_flow_and_conf
        s = TrainingSchedule(niter=1, niter_decay=1, niter_step=1, niter_fix_global=1, print_freq=2, save_latest_freq=100,
                             n_frames_total=2, n_scales_spatial=2, seq_len_max=6)
        lines = []
        left = fit(tr, seqs, s, log=lines.append)
        assert left[2] == 2 * len(seqs) and seqs.last is not None        # one step per sequence, two epochs
        for p in tr.netG[0].parameters():
            assert bool(torch.isfinite(p).all())
        print(f"pipeline: two epochs of fit over FolderSequences ran ({left})")


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    step = sys.argv[1]
    assert torch.cuda.is_available()
    globals()["step_" + step](torch.device("cuda:0"))
    torch.cuda.synchronize()
    print(f"step {step} ok", flush=True)
