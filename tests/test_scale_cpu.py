"""CPU tests of frame scaling (ir2rgb_amd.transform): the integer restatement of Pillow's 8-bit bicubic resampler and the
reference's parameter choice, against goldens recorded from Pillow and from the reference's own get_img_params
(tests/golden/make_scale_goldens.py).  Every comparison is equality: the tables are IEEE double in Pillow's operation order
and everything after them is integer arithmetic.  No GPU, no launch."""
import json
import os
import random

import numpy as np
import pytest
import torch

from ir2rgb_amd import _lib
from ir2rgb_amd import transform as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BITS = 22


@pytest.fixture(scope="module")
def goldens():
    d = np.load(os.path.join(GOLDEN, "scale_cases.npz"))
    return d, json.loads(str(d["cases"]))


@pytest.fixture(scope="module")
def built_lib():
    from ir2rgb_amd import build
    return build.build()


def restatement(img, new_size, nudge=0, offset=1 << (BITS - 1), float_between=False, sums=None):
    """A copy of the algorithm (numpy, int64 sums) with three places where a fault can be injected: ``nudge`` is added to
    every output's first coefficient, ``offset`` replaces 2**21, ``float_between`` hands the vertical pass the unrounded
    horizontal result.  ``sums``: a list that receives every pass's unclamped sums."""
    def one_pass(a, axis, out_size, last):
        a = np.moveaxis(a, axis, 0)
        bounds, coeffs, _ = T.resample_coeffs(a.shape[0], out_size)
        out = np.empty((out_size,) + a.shape[1:], dtype=np.float64 if (float_between and not last) else np.int64)
        for xx, ((xmin, xmax), k) in enumerate(zip(bounds, coeffs)):
            k = np.array(k[:xmax], dtype=np.int64)
            k[0] += nudge
            acc = np.tensordot(k.astype(a.dtype) if a.dtype == np.float64 else k, a[xmin:xmin + xmax], axes=(0, 0))
            if sums is not None:
                sums.append(np.asarray(acc))
            if float_between and not last:
                out[xx] = (acc + offset) / 2.0 ** BITS
            else:
                out[xx] = np.clip(np.floor((acc + offset) / 2.0 ** BITS) if a.dtype == np.float64 else (acc + offset) >> BITS, 0, 255)
        return np.moveaxis(out, 0, axis)

    a = np.asarray(img).astype(np.int64)
    new_w, new_h = new_size
    need_v = new_h != a.shape[0]
    if new_w != a.shape[1]:
        a = one_pass(a, 1, new_w, last=not need_v)
    if need_v:
        a = one_pass(a, 0, new_h, last=True)
    return np.clip(a, 0, 255).astype(np.uint8)


def windowed(a, m):
    x, y, w, h = T.output_window(m["new_size"], m["crop_size"], m["crop_pos"])
    a = a[y:y + h, x:x + w]
    return a[:, ::-1] if m["flip"] else a


def test_restatement_equals_every_golden(goldens):
    d, cases = goldens
    assert len(cases) >= 20 and str(d["pillow_version"])
    for m in cases:
        for c in (1, 3):
            src, want = d[f"{m['name']}/c{c}/src"], d[f"{m['name']}/c{c}/out"]
            got = T.transform_reference(torch.from_numpy(src), m["new_size"], m["crop_size"], m["crop_pos"], m["flip"])
            assert tuple(got.shape) == want.shape, (m["name"], c)
            assert np.array_equal(got.numpy(), want), (m["name"], c)
            assert np.array_equal(windowed(restatement(src[0], m["new_size"]), m), want[0]), (m["name"], c)
            one = T.transform_reference(torch.from_numpy(src[0]), m["new_size"], m["crop_size"], m["crop_pos"], m["flip"])
            assert np.array_equal(one.numpy(), want[0])                    # [H,W,C] as well as [N,H,W,C]
    gray = torch.from_numpy(d["up_dword/c1/src"][0, :, :, 0])
    assert np.array_equal(T.resize_reference(gray, (96, 64)).numpy(), d["up_dword/c1/out"][0, :, :, 0])    # [H,W]


def test_coefficient_tables_have_pillows_shape():
    for n_in, n_out, ksize in ((53, 96, 5), (96, 64, 7), (64, 32, 9), (70, 9, 33), (50, 1, 201), (1, 12, 5), (640, 1024, 5)):
        bounds, coeffs, k = T.resample_coeffs(n_in, n_out)
        assert k == ksize and len(bounds) == len(coeffs) == n_out
        for (xmin, xmax), row in zip(bounds, coeffs):
            assert 0 <= xmin and 1 <= xmax <= k and xmin + xmax <= n_in and len(row) == k
            assert all(v == 0 for v in row[xmax:])
            assert abs(sum(row) - (1 << BITS)) <= xmax                     # normalised weights, each rounded once
        assert [b[0] for b in bounds] == sorted(b[0] for b in bounds)
        assert [b[0] + b[1] for b in bounds] == sorted(b[0] + b[1] for b in bounds)
    with pytest.raises(ValueError):
        T.resample_coeffs(0, 4)


def test_restatement_equals_live_pillow_at_camera_size():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(7)
    for c in (1, 3):
        src = rng.integers(0, 256, (512, 640, c), dtype=np.uint8)
        img = Image.fromarray(src[..., 0] if c == 1 else src)
        for H, W in ((832, 1024), (512, 1024), (256, 320)):
            want = np.asarray(img.resize((W, H), Image.BICUBIC)).reshape(H, W, c)
            assert np.array_equal(T.resize_reference(torch.from_numpy(src), (W, H)).numpy(), want), (c, H, W)


def test_img_params_equal_the_references():
    with open(os.path.join(GOLDEN, "img_params_cases.json")) as f:
        records = json.load(f)["records"]
    assert len(records) >= 100
    seen = set()
    for r in records:
        random.seed(r["seed"])
        np.random.seed(r["seed"])
        p = T.img_params(r["size"], **r["opt"])
        for k in ("new_size", "crop_size", "crop_pos"):
            assert list(p[k]) == r[k] and all(type(v) is int for v in p[k]), (r, p)
        assert p["flip"] is r["flip"], (r, p)
        assert p["apply_flip"] is False                                    # neither is_train nor flip was given
        assert p["apply_crop"] is (r["opt"]["dataset_crop"] != "none")
        want = [r["opt"]["load_size"]] * 2 if r["opt"]["dataset_scale"] == "resize" else r["new_size"]
        assert list(p["scale_size"]) == want
        seen.add((tuple(r["size"]), r["opt"]["dataset_scale"], r["opt"]["dataset_crop"]))
    assert len(seen) == 3 * 4 * 3                                          # three sizes, every supported scale and crop mode
    # a seeded generator pair gives the same draws as the seeded modules
    r = next(r for r in records if r["opt"]["dataset_scale"] == "random-scale-width" and r["opt"]["dataset_crop"] == "crop")
    py, npr = random.Random(r["seed"]), np.random.RandomState(r["seed"])
    p = T.img_params(r["size"], rng=(py, npr), **r["opt"])
    assert list(p["new_size"]) == r["new_size"] and list(p["crop_pos"]) == r["crop_pos"] and p["flip"] is r["flip"]


def test_img_params_flip_none_and_the_unsupported_mode():
    opt = dict(dataset_scale="scale-width", dataset_crop="none", load_size=512, fine_size=256, dataset_mode="ir2rgb")
    draws = []
    for seed in range(8):
        random.seed(seed)
        p = T.img_params((640, 512), is_train=True, flip=True, **opt)
        assert p["apply_flip"] is p["flip"]
        random.seed(seed)
        assert T.img_params((640, 512), is_train=False, flip=True, **opt)["apply_flip"] is False
        random.seed(seed)
        assert T.img_params((640, 512), is_train=True, flip=False, **opt)["apply_flip"] is False
        draws.append(p["flip"])
    assert True in draws and False in draws
    # 'none': the size unchanged, then the reference's rounding (multiple of 4, then of 32 because nothing is cropped)
    p = T.img_params((517, 389), dataset_scale="none", dataset_crop="none", dataset_mode="ir2rgb")
    assert p["new_size"] == (512, 384) and p["scale_size"] == (512, 384) and p["crop_size"] == (0, 0)
    p = T.img_params((517, 389), dataset_scale="none", dataset_crop="crop", fine_size=250, dataset_mode="ir2rgb")
    assert p["new_size"] == (516, 388) and p["crop_size"] == (256, 256)
    with pytest.raises(ValueError, match="AttributeError in the reference"):
        T.img_params((640, 512), dataset_scale="random-scale-height", dataset_crop="none", load_size=512, fine_size=256)
    with pytest.raises(ValueError):
        T.img_params((640, 512), dataset_scale="stretch", dataset_crop="none")


def test_workspace_query_is_the_hand_stated_byte_count(goldens, built_lib):
    """The workspace holds, per frame, the horizontally scaled source rows that the kept output rows read, kept columns
    only: rows x Wc x C bytes, rows from the first kept row's window start to the last kept row's window end."""
    _, cases = goldens
    # rows x kept columns per frame and channel, by hand.  Uncropped outputs read every source row (the first window starts
    # at row 0, the last ends at the last row).  64 -> 80 rows (scale 0.8, support 2): output rows 8..71 read from
    # int(8.5 * 0.8 - 2 + 0.5) = 5 to int(71.5 * 0.8 + 2 + 0.5) = 59, i.e. 54 rows; rows 40..79 read from
    # int(40.5 * 0.8 - 1.5) = 30 to min(int(79.5 * 0.8 + 2.5), 64) = 64, i.e. 34 rows of the 50 columns 70..119.  With the
    # vertical pass skipped the workspace holds the kept rows themselves.
    hand = {"up_dword": 37 * 96, "up_scalar": 37 * 95, "down_9_7_taps": 64 * 64, "down_33_taps": 50 * 9, "down_to_1x1": 50 * 1,
            "narrow_source": 9 * 128, "from_1x1": 1 * 12, "skip_vertical": 33 * 96, "skip_horizontal": 33 * 47,
            "skip_both": 33 * 47, "crop": 54 * 64, "crop_off_edge": 34 * 50, "crop_larger_than_image": 64 * 120,
            "flip": 64 * 120, "flip_crop": 54 * 64, "skip_both_flip_crop": 16 * 32, "checker_down": 63 * 53,
            "checker_up": 37 * 96, "steps_down": 63 * 53, "steps_up": 37 * 96}
    assert set(hand) == {m["name"] for m in cases}
    for m in cases:
        hs, ws = m["src_hw"]
        nw, nh = m["new_size"]
        x, y, wc, hc = T.output_window(m["new_size"], m["crop_size"], m["crop_pos"])
        if nh == hs:
            rows = hc
        else:
            b = T.resample_coeffs(hs, nh)[0]
            rows = max(lo + n for lo, n in b[y:y + hc]) - min(lo for lo, _ in b[y:y + hc])
        for c in (1, 3):
            for n in (1, 3):
                got = _lib.query("ir2rgb_frame_scale_workspace_bytes", n, c, hs, ws, nh, nw, y, x, hc, wc)
                assert got == n * rows * wc * c, (m["name"], c, n)
                assert got == n * c * hand[m["name"]], (m["name"], c, n)
    # a crop: output rows 8..71 of 64 -> 80 read from the start of row 8's window to the end of row 71's
    b = T.resample_coeffs(64, 80)[0]
    assert _lib.query("ir2rgb_frame_scale_workspace_bytes", 1, 3, 64, 96, 80, 120, 8, 16, 64, 64) == \
        (b[71][0] + b[71][1] - b[8][0]) * 64 * 3
    for bad in ((0, 3, 8, 8, 8, 8, 0, 0, 8, 8), (1, 2, 8, 8, 8, 8, 0, 0, 8, 8), (1, 3, 8, 8, 16, 16, 9, 0, 8, 8),
                (1, 3, 8, 8, 16, 16, 0, -1, 8, 8), (1, 3, 8, 8, 16, 16, 0, 0, 0, 8)):
        assert _lib.lib().ir2rgb_frame_scale_workspace_bytes(*bad) == -1
        with pytest.raises(ValueError, match="frame_scale_workspace_bytes"):
            _lib.query("ir2rgb_frame_scale_workspace_bytes", *bad)


def test_launch_arguments_are_validated_before_anything_runs(built_lib):
    """ir2rgb_frame_scale_u8 refuses bad arguments before any launch (no GPU here): both bindings, same codes."""
    lib = _lib.lib()
    t = torch.zeros(4096, dtype=torch.int32)
    p = t.data_ptr()
    geom = (1, 3, 8, 8, 16, 16, 0, 0, 16, 16)
    ok_tables = (p, p, 5, p, p, 5)
    call = lambda *a: lib.ir2rgb_frame_scale_u8(*a, None)      # noqa: E731
    assert call(None, p, p, 1 << 20, *ok_tables, *geom, 0, 0) == -1                    # NULL source
    assert call(p, p, p, 8 * 16 * 3 - 1, *ok_tables, *geom, 0, 0) == -1                # workspace too small
    assert call(p, p, p, 1 << 20, p, p, 7, p, p, 5, *geom, 0, 0) == -1                 # ksize of another scale
    assert call(p, p, p, 1 << 20, None, None, 0, p, p, 5, *geom, 0, 0) == -1           # tables missing
    assert call(p, p, p, 1 << 20, p, p, 5, p, p, 5, 1, 3, 8, 16, 16, 16, 0, 0, 16, 16, 0, 0) == -1    # tables for a skipped pass
    assert call(p, p, p, 1 << 20, *ok_tables, *geom, 2, 0) == -1                       # flip is 0 / 1
    assert call(p, p, p, 1 << 20, p + 2, p, 5, p, p, 5, *geom, 0, 0) == -3             # misaligned table
    assert call(p, p + 1, p, 1 << 20, *ok_tables, *geom, 0, 1) == -3                   # misaligned fp32 destination


FAULTS = {"coefficient off by 1": dict(nudge=1), "offset 2**21 - 1": dict(offset=(1 << (BITS - 1)) - 1),
          "float between the passes": dict(float_between=True)}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_an_injected_fault_changes_a_golden(goldens, fault):
    d, cases = goldens
    changed = []
    for m in cases:
        for c in (1, 3):
            got = windowed(restatement(d[f"{m['name']}/c{c}/src"][0], m["new_size"], **FAULTS[fault]), m)
            if not np.array_equal(got, d[f"{m['name']}/c{c}/out"][0]):
                changed.append((m["name"], c))
    assert changed, f"no golden output notices: {fault}"


def test_saturating_cases_exercise_the_clamp_on_both_sides(goldens):
    d, cases = goldens
    sat = [m for m in cases if m["saturating"]]
    assert len(sat) == 4
    for m in sat:
        for c in (1, 3):
            sums = []
            restatement(d[f"{m['name']}/c{c}/src"][0], m["new_size"], sums=sums)
            lo, hi = min(int(s.min()) for s in sums), max(int(s.max()) for s in sums)
            assert lo + (1 << (BITS - 1)) < 0 and (hi + (1 << (BITS - 1))) >> BITS > 255, (m["name"], c, lo, hi)
            assert lo < 0 and hi > 255 << BITS
            assert abs(lo) < 2 ** 31 and hi < 2 ** 31                        # the int32 accumulator holds every sum
            out = d[f"{m['name']}/c{c}/out"]
            assert out.min() == 0 and out.max() == 255
