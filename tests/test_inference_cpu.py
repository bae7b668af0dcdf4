"""CPU side of frame-by-frame inference (ir2rgb_amd.inference, csrc/frame_io.hip): the frame-I/O arithmetic pinned by
numpy / torch restatements (what tests/test_inference_gpu.py holds the kernels to, exactly), the golden files, the host
logic that needs no GPU, and the presence of the new entry points in every table."""
import glob
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = ("1scale_ngf64_zeros", "2scale_ngf128_real", "2scale_ngf128_real_eval")


# ---------------------------------------------------------------------------------------------
# the restatements (imported by tests/test_inference_gpu.py)
# ---------------------------------------------------------------------------------------------
def push_restatement(frame_u8):
    """transforms.ToTensor + Normalize(0.5, 0.5) (reference data/transform.py:82-85) of a uint8 [H,W,C] frame ->
    fp32 [C,H,W]: ToTensor is ``.float().div(255)`` of the CHW bytes, Normalize ``.sub(mean).div(std)``."""
    return torch.as_tensor(frame_u8).permute(2, 0, 1).contiguous().float().div(255).sub(0.5).div(0.5)


def pool_restatement(planes):
    """build_pyr's down-sampling (base_model.py:77): fp32 [...,H,W] -> [...,(H-1)//2+1,(W-1)//2+1]."""
    p = planes.reshape((-1, 1) + tuple(planes.shape[-2:]))
    y = torch.nn.functional.avg_pool2d(p, 3, stride=2, padding=1, count_include_pad=False)
    return y.reshape(tuple(planes.shape[:-2]) + tuple(y.shape[-2:]))


def finish_restatement(image):
    """util.tensor2im (reference util/util.py:59-68) of an fp32 [3,H,W] tensor -> uint8 [H,W,3], numpy as the reference."""
    image_numpy = torch.as_tensor(image).cpu().float().numpy()
    image_numpy = (np.transpose(image_numpy, (1, 2, 0)) + 1) / 2.0 * 255.0
    image_numpy = np.clip(image_numpy, 0, 255)
    return image_numpy.astype(np.uint8)


def shift_restatement(hist, new):
    """torch.cat([prev[1:], fake_B]) (generator.py:214)."""
    return torch.cat([hist[1:], new.reshape((1,) + tuple(hist.shape[1:]))])


def finish_grid():
    """Values that decide the uint8 conversion: the ends, beyond them, and for every byte b the fp32 numbers around the
    point where (x + 1) / 2 * 255 crosses b and b + 0.5."""
    pts = [-1.0, 1.0, -1.5, 1.5, -3.0, 7.0, 0.0, -0.0]
    for b in range(256):
        for t in (b, b + 0.5):
            x = np.float32(t / 255.0 * 2.0 - 1.0)
            pts += [x, np.nextafter(x, np.float32(-4)), np.nextafter(x, np.float32(4))]
    return torch.tensor(np.array(pts, dtype=np.float32))


# ---------------------------------------------------------------------------------------------
# arithmetic
# ---------------------------------------------------------------------------------------------
def test_normalisation_of_all_256_bytes():
    from ir2rgb_amd import inference as I
    want = torch.stack([torch.tensor(v, dtype=torch.uint8).float().div(255).sub(0.5).div(0.5) for v in range(256)])
    frame = torch.arange(256, dtype=torch.uint8).view(16, 16, 1)
    assert torch.equal(push_restatement(frame).flatten(), want)
    assert torch.equal(I.normalise_u8(frame).flatten(), want)
    assert want[0] == -1 and want[255] == 1 and bool((want[1:] > want[:-1]).all())
    # a 3-channel frame: the interleaved bytes land in their planes
    rgb = torch.arange(2 * 4 * 3, dtype=torch.uint8).view(2, 4, 3)
    got = push_restatement(rgb)
    assert got.shape == (3, 2, 4) and torch.equal(got[1, 1, 2], want[int(rgb[1, 2, 1])])


def test_uint8_conversion_on_the_deciding_grid():
    from ir2rgb_amd import inference as I
    g = finish_grid()
    n = g.numel()
    pad = (-n) % 4
    x = torch.cat([g, g.new_zeros(pad)]).view(1, -1, 4).expand(3, -1, -1).contiguous()
    want = finish_restatement(x)
    # the same expression spelt out per element in numpy float32, truncation toward zero
    v = np.clip((x.numpy().transpose(1, 2, 0) + np.float32(1)) / np.float32(2) * np.float32(255), 0, 255)
    assert v.dtype == np.float32 and np.array_equal(want, np.trunc(v).astype(np.uint8))
    assert np.array_equal(I.to_u8(x).numpy(), want)
    flat = want[:, :, 0].reshape(-1)[:n]
    assert flat[0] == 0 and flat[1] == 255 and flat[2] == 0 and flat[3] == 255 and flat[4] == 0 and flat[5] == 255
    assert flat[6] == 127                       # (0 + 1) / 2 * 255 = 127.5 truncates
    assert set(np.unique(flat)) == set(range(256))


def test_pool_restatement_counts_only_valid_pixels():
    x = torch.arange(5 * 6, dtype=torch.float32).view(1, 5, 6)
    y = pool_restatement(x)
    assert y.shape == (1, 3, 3)
    assert y[0, 0, 0] == x[0, :2, :2].mean() and y[0, 1, 1] == x[0, 1:4, 1:4].mean() and y[0, 2, 2] == x[0, 3:5, 3:6].mean()


def test_history_shift_restatement():
    h = torch.arange(3 * 2, dtype=torch.float32).view(3, 2)
    out = shift_restatement(h, torch.tensor([9.0, 9.0]))
    assert torch.equal(out, torch.tensor([[2.0, 3.0], [4.0, 5.0], [9.0, 9.0]]))


# ---------------------------------------------------------------------------------------------
# goldens
# ---------------------------------------------------------------------------------------------
def load_golden_helpers():
    spec = importlib.util.spec_from_file_location("make_infer_goldens", os.path.join(GOLDEN, "make_infer_goldens.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)            # defines helpers only; the reference is imported inside main()
    return mod


@pytest.mark.parametrize("tag", CASES)
def test_golden_files_carry_frames_and_floors(tag):
    path = os.path.join(GOLDEN, f"infer_{tag}.npz")
    assert os.path.exists(path)
    biggest = max(os.path.getsize(p) for p in glob.glob(os.path.join(GOLDEN, "window_*.npz")))
    assert os.path.getsize(path) <= min(biggest, 1 << 20)
    d = np.load(path)
    ns, n_gen = int(d["n_scales"]), 6
    assert d["ir_u8"].dtype == np.uint8 and d["ir_u8"].shape == (8, 64, 128, 3)
    assert (str(d["first_frame"]) == "real") == ("rgb_u8" in d.files)
    assert bool(d["eval_mode"]) == tag.endswith("_eval")
    for i in range(ns):
        h, w = 64 >> i, 128 >> i
        for kind in ("free", "tf"):
            a = d[f"{kind}/s{i}"]
            assert a.shape == (n_gen, 3, h, w) and np.isfinite(a.astype(np.float32)).all()
            assert np.abs(a.astype(np.float32)).max() <= 1.0 + 1e-3         # tanh images and their blends
        for name in ("bf16", "f16"):
            f = d[f"floor/{name}/s{i}"]
            assert f.shape == (n_gen,) and (f > 0).all() and (f < 1.0).all(), (name, f)
        assert d["floor/f16/s0"].mean() < d["floor/bf16/s0"].mean()       # three more mantissa bits


@pytest.mark.parametrize("tag", CASES)
def test_free_running_and_teacher_forced_frames_differ_only_through_the_history(tag):
    """Frame 0 starts from the first-frame rule (exact on both sides): identical.  Later frames start from the stored
    (float16) history in the teacher-forced run and from the fp32 one in the free-running loop: close, not identical."""
    M = load_golden_helpers()
    d = np.load(os.path.join(GOLDEN, f"infer_{tag}.npz"))
    for i in range(int(d["n_scales"])):
        free, tf = d[f"free/s{i}"].astype(np.float32), d[f"tf/s{i}"].astype(np.float32)
        assert np.array_equal(free[0], tf[0])
        rel = [np.linalg.norm(free[t] - tf[t]) / np.linalg.norm(free[t]) for t in range(1, free.shape[0])]
        assert max(rel) < 0.05, rel
        assert not np.array_equal(free[1:], tf[1:]) or bool(d["eval_mode"])
        # the history of frame t is the two free-running frames before it (first-frame rule in front)
        h2 = M.history(d, 3)[i]
        assert torch.equal(h2, torch.as_tensor(d[f"free/s{i}"][1:3]).float())
        h0 = M.history(d, 0)[i]
        if str(d["first_frame"]) == "zeros":
            assert h0.shape == h2.shape and not h0.any()
        else:
            want = push_restatement(d["rgb_u8"][0])
            for _ in range(i):
                want = pool_restatement(want)
            assert torch.equal(h0[0], want)
        assert torch.equal(M.history(d, 1)[i][1], torch.as_tensor(d[f"free/s{i}"][0]).float())


# ---------------------------------------------------------------------------------------------
# host logic
# ---------------------------------------------------------------------------------------------
def test_translator_refuses_cpu_and_dead_branches():
    import ir2rgb_amd
    from ir2rgb_amd.inference import VideoTranslator
    assert ir2rgb_amd.VideoTranslator is VideoTranslator
    with pytest.raises(ValueError, match="no CPU fallback"):
        VideoTranslator(torch.device("cpu"), 64, 128)
    with pytest.raises(ValueError, match="no CPU fallback"):
        VideoTranslator("cpu", 64, 128)
    with pytest.raises(NotImplementedError, match="dead branch for IR->RGB"):
        VideoTranslator("cuda:0", 64, 128, fg=True)
    with pytest.raises(NotImplementedError, match="dead branch for IR->RGB"):
        VideoTranslator("cuda:0", 64, 128, use_single_G=True)
    with pytest.raises(ValueError, match="first_frame"):
        VideoTranslator("cuda:0", 64, 128, first_frame="single")
    with pytest.raises(ValueError, match="norm_stats"):
        VideoTranslator("cuda:0", 64, 128, norm_stats="folded")
    with pytest.raises(TypeError, match="unknown options"):
        VideoTranslator("cuda:0", 64, 128, n_scale_spatial=2)


def test_warm_up_counting_and_reset():
    from ir2rgb_amd.inference import SequenceState
    for tG in (2, 3, 4):
        s = SequenceState(tG)
        assert [s.push() for _ in range(tG + 2)] == [False] * (tG - 1) + [True] * 3     # no frame for the first tG-1
        assert s.begin_step() is True and s.begin_step() is False                         # one first frame per sequence
        s.reset()
        assert s.n_pushed == 0 and not s.started and s.warming
        assert [s.push() for _ in range(tG)] == [False] * (tG - 1) + [True]
        assert s.begin_step() is True


# ---------------------------------------------------------------------------------------------
# the entry points are declared, bound and wrapped
# ---------------------------------------------------------------------------------------------
def test_entry_points_are_present_everywhere():
    from ir2rgb_amd import _lib, fastbind
    names = ("ir2rgb_frame_push_u8", "ir2rgb_frame_finish_u8")
    header = open(os.path.join(ROOT, "include", "ir2rgb_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for n in names:
        assert re.search(r"\bint\s+%s\s*\(" % n, header)
        assert n in _lib.PROTOTYPES and n in fastbind.wrappable()
    assert os.path.exists(os.path.join(ROOT, "ir2rgb_amd", "csrc", "frame_io.hip"))


def test_bad_arguments_are_refused_before_any_launch():
    from ir2rgb_amd import build, _lib
    build.build()
    lib = _lib.lib()
    buf = torch.zeros(4096)
    p = buf.data_ptr()
    assert lib.ir2rgb_frame_push_u8(p, p, None, 3, 2, 4, 4, 0, None) == -1           # C not in {1, 3}
    assert lib.ir2rgb_frame_push_u8(None, p, None, 3, 3, 4, 4, 0, None) == -1
    assert lib.ir2rgb_frame_push_u8(p, p, None, 0, 3, 4, 4, 0, None) == -1
    assert lib.ir2rgb_frame_push_u8(p, p + 2, None, 3, 3, 4, 4, 0, None) == -3       # fp32 history on a 2-byte boundary
    assert lib.ir2rgb_frame_finish_u8(p, None, None, 2, 4, 4, None) == -1
    assert lib.ir2rgb_frame_finish_u8(p, p, None, 2, 0, 4, None) == -1
    assert lib.ir2rgb_frame_finish_u8(p + 1, p, None, 2, 4, 4, None) == -3
