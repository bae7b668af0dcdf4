"""CPU side of the training snapshots (ir2rgb_amd/visuals.py): the definitions against the reference's own results, the
integer HSV stage against an independent formulation, the conditions the GPU comparison rests on, and the file layer.

What is pinned by what:
  * ``to_u8_reference`` and ``panels``: tests/golden/visuals_*.npz, recorded from the reference's ``tensor2im`` and
    ``save_all_tensors`` (tests/golden/make_visuals_goldens.py), tolerance 0;
  * the flow coding: NOT by the reference (its ``tensor2flow`` goes through OpenCV, which is not available to make a
    fixture).  Its integer stage is held to Python's ``colorsys`` over all 180 x 256 inputs; its float stage is the
    documented formula in fp64, and five planted faults show that the comparison on the GPU test's inputs would see a
    wrong one.
"""
import colorsys
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import visuals_inputs as VI  # noqa: E402

from ir2rgb_amd import visuals as V  # noqa: E402


# ---------------------------------------------------------------------------------------------
# against the reference's results
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def im_golden(golden_dir):
    return np.load(os.path.join(golden_dir, "visuals_tensor2im.npz"))


@pytest.fixture(scope="module")
def panel_golden(golden_dir):
    return np.load(os.path.join(golden_dir, "visuals_panels.npz"))


def _keys(g):
    return sorted({k.rsplit("/", 1)[0] for k in g.files})


def test_to_u8_reference_against_tensor2im(im_golden):
    g = im_golden
    keys = _keys(g)
    assert len(keys) == 8 and {k for k in keys if k.startswith("boundary")} == {"boundary_c1", "boundary_c3"}
    for key in keys:
        x = torch.from_numpy(g[key + "/x"])
        for mode, normalize in (("norm", True), ("unit", False)):
            got, want = V.to_u8_reference(x, normalize), g[f"{key}/{mode}"]
            assert got.dtype == np.uint8 and got.shape == want.shape, (key, mode, got.shape, want.shape)
            assert np.array_equal(got, want), (key, mode, int((got != want).sum()))
    # the random inputs reach past both ends, the boundary inputs hold every byte value
    assert (g["rand_c3_d5/x"] < -1).any() and (g["rand_c3_d5/x"] > 1).any()
    assert set(np.unique(g["boundary_c1/norm"])) == set(range(256)) == set(np.unique(g["boundary_c1/unit"]))


def test_rounding_instead_of_truncation_changes_a_golden(im_golden, monkeypatch):
    """The planted fault of the 8-bit conversion: ``round`` for ``trunc`` moves bytes of the boundary inputs."""
    x = torch.from_numpy(im_golden["boundary_c3/x"])
    monkeypatch.setattr(V, "_TO_INTEGER", np.rint)
    for mode, normalize in (("norm", True), ("unit", False)):
        got = V.to_u8_reference(x, normalize)
        assert (got != im_golden[f"boundary_c3/{mode}"]).mean() > 0.1, mode


def test_panels_against_save_all_tensors(panel_golden):
    g = panel_golden
    for input_nc in (1, 3):
        for with_flow in (0, 1):
            key = f"nc{input_nc}_flow{with_flow}"
            t = {k: (torch.from_numpy(g[f"{key}/in/{k}"]) if f"{key}/in/{k}" in g.files else None)
                 for k in ("real_A", "fake_B", "fake_B_first", "fake_B_raw", "real_B", "flow_ref", "conf_ref", "flow", "weight")}
            plist = V.panels(t, {"input_nc": input_nc})
            assert [n for n, _, _ in plist] == [str(n) for n in g[key + "/names"]]
            assert len(plist) == (9 if with_flow else 7)
            assert [n for n, kind, _ in plist if kind == V.FLOW] == [str(n) for n in g[key + "/flow_names"]]
            for n, kind, x in plist:
                assert x.dim() == 3 and x.is_contiguous() and x.shape[0] == (2 if kind == V.FLOW else x.shape[0])
            images = V.reference_images(plist)
            for n, kind, x in plist:
                if kind != V.FLOW:
                    want = g[f"{key}/out/{n}"]
                    assert images[n].shape == want.shape and np.array_equal(images[n], want), (key, n)
            # the reference's quirk and the alternative
            assert plist[0][:2] == ("input_image", V.IMAGE_UNIT) and plist[0][2].shape[0] == input_nc
            alt = V.panels(t, {"input_nc": input_nc}, input_panel="normalised")
            assert alt[0][1] == V.IMAGE_NORM and [p[:2] for p in alt[1:]] == [p[:2] for p in plist[1:]]
    with pytest.raises(ValueError):
        V.panels(t, {"input_nc": 3}, input_panel="other")


def test_lazy_exports():
    import ir2rgb_amd
    assert ir2rgb_amd.Snapshots is V.Snapshots and ir2rgb_amd.to_u8_reference is V.to_u8_reference
    assert ir2rgb_amd.flow_to_rgb_reference is V.flow_to_rgb_reference


# ---------------------------------------------------------------------------------------------
# bytes to RGB: every input against colorsys
# ---------------------------------------------------------------------------------------------
def test_hsv_bytes_to_rgb_exhaustively_against_colorsys():
    hb, vb = np.meshgrid(np.arange(180), np.arange(256), indexing="ij")
    got = V.hsv_bytes_to_rgb(hb, vb).astype(np.int64)
    exact = np.array([[[c * 255.0 for c in colorsys.hsv_to_rgb(h / 180.0, 1.0, v / 255.0)] for v in range(256)] for h in range(180)])
    frac = exact - np.floor(exact)
    clear = np.abs(frac - 0.5) > 1e-9
    want = np.floor(exact + 0.5).astype(np.int64)
    assert clear.mean() > 0.9
    assert np.array_equal(got[clear], want[clear])
    assert np.abs(got - exact).max() <= 1.0 and (np.abs(got - want) <= 1).all()
    assert np.array_equal(V.hsv_bytes_to_rgb(np.full(256, 180), np.arange(256)), V.hsv_bytes_to_rgb(np.zeros(256, int), np.arange(256)))


# ---------------------------------------------------------------------------------------------
# the flow coding on the GPU test's inputs
# ---------------------------------------------------------------------------------------------
def coded(flow, fault=None):
    """The floats-to-bytes stage written out once more, in fp64, with one of the planted faults -> rgb."""
    f = flow.numpy().astype(np.float64)
    u, v = (f[1], f[0]) if fault == "uv_swapped" else (f[0], f[1])
    mag = np.sqrt(u * u + v * v)
    ang = np.arctan2(v, u)
    ang = np.where(ang < 0, ang + 2 * np.pi, ang)
    h = ang * 180 / np.pi / (1 if fault == "angle_not_halved" else 2)
    hb = np.trunc(h).astype(np.int64) % 180
    mn, mx = mag.min(), mag.max()
    if fault == "range_over_u":
        rng = np.abs(u).max() - np.abs(u).min()
    else:
        rng = mx - mn
    if mx == mn:
        vb = np.zeros(mag.shape, dtype=np.int64)
    else:
        val = (mag - (0.0 if fault == "min_not_subtracted" else mn)) * 255 / rng
        vb = np.trunc(np.clip(val, 0, 255)).astype(np.int64)
    rgb = V.hsv_bytes_to_rgb(hb, vb)
    return rgb[..., ::-1] if fault == "r_b_exchanged" else rgb


@pytest.fixture(scope="module")
def flow_panels():
    return VI.random_flow_panels()


def test_flow_inputs_are_decided(flow_panels):
    """The condition the GPU comparison needs: almost every pixel of every random flow panel is decided, so that the
    byte-for-byte comparison covers it.  The pixels of smallest and largest magnitude are never decided (their scaled
    values are the integers 0 and 255 by construction), which at 15 pixels is more than 1 %: the condition is 99 % of the
    other pixels, and 99 % of all pixels where a panel is large enough for that to be possible (200 pixels).  A constant
    panel (one pixel) is decided everywhere and black."""
    assert len(flow_panels) == 5 * (2 + 1 + 2)
    for case, key, flow in flow_panels:
        rgb, decided, hb, vb = V.flow_to_rgb_reference(flow)
        n = decided.size
        if n == 1:
            assert decided.all() and not rgb.any(), (case, key)
            continue
        mag = flow.double().pow(2).sum(0).sqrt().reshape(-1)
        assert not decided.reshape(-1)[[int(mag.argmin()), int(mag.argmax())]].any()
        assert decided.sum() >= 0.99 * (n - 2), (case, key, int(decided.sum()), n)
        if n >= 200:
            assert decided.mean() >= 0.99, (case, key, decided.mean())
        assert np.array_equal(rgb, coded(flow)), (case, key)          # the module's reference is that formula


@pytest.mark.parametrize("fault", ["uv_swapped", "angle_not_halved", "min_not_subtracted", "range_over_u", "r_b_exchanged"])
def test_planted_flow_faults_change_the_decided_pixels(flow_panels, fault):
    changed = total = 0
    for case, key, flow in flow_panels:
        rgb, decided, _, _ = V.flow_to_rgb_reference(flow)
        if decided.size == 1:
            continue                    # (black whatever the formula)
        diff = (coded(flow, fault) != rgb).any(-1) & decided
        assert diff.sum() > 0.1 * decided.sum(), (fault, case, key, int(diff.sum()), int(decided.sum()))
        changed, total = changed + int(diff.sum()), total + int(decided.sum())
    assert changed > 0.1 * total


def test_flow_reference_exact_cases():
    z = torch.zeros(2, 3, 4)
    rgb, decided, _, _ = V.flow_to_rgb_reference(z)
    assert not rgb.any() and decided.all()
    c = torch.stack([torch.full((3, 4), 1.5), torch.full((3, 4), -2.0)])
    rgb, decided, _, _ = V.flow_to_rgb_reference(c)
    assert not rgb.any() and decided.all()
    nan = float("nan")
    f = torch.tensor([[1.0, 0.0, -1.0, 0.0, 0.0, nan], [0.0, 1.0, 0.0, -1.0, 0.0, 1.0]]).view(2, 1, 6)
    rgb, _, hb, vb = V.flow_to_rgb_reference(f)
    assert hb[0, :4].tolist() == [0, 45, 90, 135] and vb[0].tolist() == [255, 255, 255, 255, 0, 0]
    assert rgb[0].tolist() == [[255, 0, 0], [128, 255, 0], [0, 255, 255], [128, 0, 255], [0, 0, 0], [0, 0, 0]]
    # tensor2flow's indexing
    assert np.array_equal(V.flow_to_rgb_reference(f.view(1, 2, 1, 6).expand(2, 2, 1, 6))[0], rgb)
    with pytest.raises(ValueError):
        V.flow_to_rgb_reference(torch.zeros(3, 2, 2))


# ---------------------------------------------------------------------------------------------
# files
# ---------------------------------------------------------------------------------------------
NINE = [("input_image", 3), ("fake_image", 3), ("fake_first_image", 3), ("fake_raw_image", 3), ("real_image", 3), ("flow_ref", 2),
        ("conf_ref", 1), ("flow", 2), ("weight", 1)]


def test_file_layer(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(3)
    stack = rng.integers(0, 256, (9, 6, 10, 3), dtype=np.uint8)
    for k, (_, ch) in enumerate(NINE):
        if ch == 1:
            stack[k] = stack[k][:, :, :1]
    img_dir = str(tmp_path / "images")
    for epoch in (1, 2, 12):
        V.write_images(img_dir, epoch, NINE, stack + epoch, "png")
    assert sorted(os.listdir(img_dir)) == sorted("epoch%.3d_%s.png" % (e, n) for e in (1, 2, 12) for n, _ in NINE)
    for k, (name, ch) in enumerate(NINE):
        im = Image.open(os.path.join(img_dir, "epoch012_%s.png" % name))
        assert im.mode == ("L" if ch == 1 else "RGB") and im.size == (10, 6)
        want = (stack[k] + 12)[:, :, 0] if ch == 1 else stack[k] + 12
        assert np.array_equal(np.asarray(im), want), name
    V.write_images(img_dir, 3, NINE[:2], stack, "jpg")
    assert Image.open(os.path.join(img_dir, "epoch003_fake_image.jpg")).format == "JPEG"

    labels = [n for n, _ in NINE]
    V.write_index(str(tmp_path), 3, labels, "png")
    html = open(tmp_path / "index.html").read()
    heads = [html.index("epoch [%d]" % e) for e in (3, 2, 1)]
    assert heads == sorted(heads) and "epoch [4]" not in html           # newest first
    block = html[heads[0]:heads[1]]
    rows = block.split("<table")[1:]
    assert len(rows) == 2                                                # nine panels: rows of round(9 / 2) = 4 and 5
    assert [r.count("<img ") for r in rows] == [4, 5]
    order = [block.index("images/epoch003_%s.png" % n) for n in labels]
    assert order == sorted(order)
    assert all(("images/epoch%.3d_%s.png" % (e, n)) in html for e in (1, 2, 3) for n in labels)
    V.write_index(str(tmp_path), 1, labels[:5], "jpg")                  # fewer than six: one row
    html = open(tmp_path / "index.html").read()
    assert html.count("<table") == 1 and html.count("<img ") == 5 and "epoch001_input_image.jpg" in html
    V.write_index(str(tmp_path), 1, labels[:7], "jpg")                  # seven: round(3.5) = 4 and 3
    html = open(tmp_path / "index.html").read()
    assert [r.count("<img ") for r in html.split("<table")[1:]] == [4, 3]


def test_snapshots_arguments():
    with pytest.raises(ValueError):
        V.Snapshots("cpu", "x", freq=0)
    with pytest.raises(ValueError):
        V.Snapshots("cpu", "x", input_panel="raw")
    s = V.Snapshots("cpu", "x", freq=3)
    assert [s.due(k) for k in (1, 2, 3, 6, 7)] == [False, False, True, True, False]
    s.flush()            # nothing pending: nothing written
    assert not os.path.exists("x")
