"""The JPEG definition on the CPU (ir2rgb_amd.jpeg.jpeg_reference): equal to Pillow's files byte for byte, live where
Pillow sits on libjpeg-turbo and against tests/golden/jpeg_cases.npz everywhere.  Every comparison is equality.

  * the grid of the goldens (three modes, q in {1, 30, 75, 95, 100}, restart_rows in {1, 2}, ten shapes from 1x1 to 144x40)
    and their extras; the counters of the paths the streams took prove that the goldens reach every rule
  * a stream with restart markers decodes to the pixels of the file without them
  * the header and the quality tables for q = 1 .. 100
  * six faults planted into the reference are each caught by some golden
  * the library refuses bad arguments before any launch (no GPU here: the pointers are never dereferenced)
"""
import io
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_jpeg_goldens as G  # noqa: E402

from ir2rgb_amd import jpeg as J  # noqa: E402


@pytest.fixture(scope="module")
def goldens():
    d = np.load(G.PATH)
    cases = json.loads(str(d["cases"]))
    files = d["files"]
    return [(m, d[m["src"]], files[m["offset"]:m["offset"] + m["length"]].tobytes()) for m in cases], json.loads(str(d["fullsize"]))


def _reference(m, src, **kw):
    return J.jpeg_reference(src, m["quality"], m["mode"], m["restart_rows"], **kw)


def _turbo():
    try:
        from PIL import features
        return bool(features.check_feature("libjpeg_turbo"))
    except Exception:
        return False


def test_golden_grid_is_the_issue_grid(goldens):
    names = {m["name"] for m, _, _ in goldens[0]}
    for h, w in [(1, 1), (8, 8), (8, 24), (24, 8), (7, 9), (13, 21), (16, 16), (17, 33), (31, 47), (144, 40)]:
        for mode in ("4:4:4", "4:2:0", "L"):
            for q in (1, 30, 75, 95, 100):
                for rr in (1, 2):
                    assert f"{h}x{w}/{mode}/q{q}/r{rr}" in names
    for mode in ("4:4:4", "4:2:0", "L"):
        assert J.Geometry(144, 40, mode, 1).n_intervals > 8
    assert [f["mode"] for f in goldens[1]] == ["4:4:4", "4:2:0", "L"]


def test_reference_equals_every_golden(goldens):
    for m, src, want in goldens[0]:
        got = _reference(m, src)
        assert len(got) == 1 and got[0] == want, m["name"]


def test_reference_equals_pillow_live(goldens):
    if not _turbo():
        return          # another libjpeg: the goldens stand in (test_reference_equals_every_golden)
    rng = np.random.default_rng(5)
    n = 0
    for h, w in G.SHAPES:
        src = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        for mode in G.MODES:
            for q in G.QUALITIES:
                for rr in (0,) + G.RESTART_ROWS:
                    assert J.jpeg_reference(src, q, mode, rr)[0] == G.pillow_file(src, mode, q, rr), (h, w, mode, q, rr)
                    n += 1
    assert n == 450
    # several frames in one call, one-channel input for mode L
    src = rng.integers(0, 256, (3, 13, 21, 1), dtype=np.uint8)
    assert J.jpeg_reference(src, 75, "L", 1) == [G.pillow_file(f, "L", 75, 1) for f in src]


def test_full_size_golden(goldens):
    import hashlib
    frame = G.fullsize_frame()
    assert frame.shape == (512, 1024, 3) and frame.min() == 0 and frame.max() == 255
    f = goldens[1][1]                                                   # 4:2:0, the default
    data = J.jpeg_reference(frame, f["quality"], f["mode"], f["restart_rows"])[0]
    assert len(data) == f["length"] and hashlib.sha256(data).hexdigest() == f["sha256"]


def test_goldens_reach_every_path(goldens):
    total = dict.fromkeys(J.COUNTERS, 0)
    for m, src, _ in goldens[0]:
        _, c = _reference(m, src, counters=True)
        for k, v in c.items():
            total[k] = max(total[k], v) if k.startswith("max_") else total[k] + v
    assert total["zrl"] > 0 and total["stuffed"] > 0
    assert total["max_dc_size"] == 11 and total["max_ac_size"] == 10        # the saturated checkerboard at q = 100
    assert total["eob_only_blocks"] > 0
    assert total["dummy_right"] > 0 and total["dummy_bottom"] > 0
    assert total["odd_h_chroma_rows"] > 0
    assert total["padded_chroma_cols_bias1"] > 0 and total["padded_chroma_cols_bias2"] > 0
    assert total["rst_wrapped"] > 0 and total["intervals"] > len(goldens[0])
    # the flat frame is nothing but EOB blocks after its first; the checkerboard alone reaches the largest sizes
    by_name = {m["name"]: (m, src) for m, src, _ in goldens[0]}
    _, c = _reference(*by_name["flat/4:2:0/q75/r1"], counters=True)
    assert c["eob_only_blocks"] == J.Geometry(17, 33, "4:2:0", 1).n_blocks
    _, c = _reference(*by_name["checker/L/q100/r1"], counters=True)
    assert (c["max_dc_size"], c["max_ac_size"]) == (11, 10)
    # an interval longer than the 128 blocks the entropy kernel takes at a time, in two modes
    assert 2 * 43 * 3 > 128 and J.Geometry(16, 344, "4:2:0", 1).n_blocks == 132


def test_restart_markers_change_no_pixel(goldens):
    from PIL import Image
    rng = np.random.default_rng(9)
    for (h, w), mode in (((31, 47), "4:2:0"), ((144, 40), "4:4:4"), ((17, 33), "L")):
        src = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        marked = J.jpeg_reference(src, 75, mode, 1)[0]
        plain = J.jpeg_reference(src, 75, mode, 0)[0]
        assert marked != plain and b"\xff\xdd" in marked and b"\xff\xdd" not in plain
        a, b = (np.asarray(Image.open(io.BytesIO(x))) for x in (marked, plain))
        assert a.shape[:2] == (h, w) and np.array_equal(a, b), mode
        if _turbo():
            assert plain == G.pillow_file(src, mode, 75, 0)


def test_header_and_quality_tables(goldens):
    for m, src, want in goldens[0]:
        head = J.header(*m["hw"], m["quality"], m["mode"], m["restart_rows"])
        assert want.startswith(head) and head.endswith(b"\x00\x3f\x00") and head.count(b"\xff\xda") == 1, m["name"]
    # jpeg_set_quality against the endpoints anyone can work out by hand, and monotone in between
    lum, chroma = J.quality_tables(50)
    assert np.array_equal(lum, J.BASE_LUMA) and np.array_equal(chroma, J.BASE_CHROMA)
    assert all((t == 1).all() for t in J.quality_tables(100)) and J.quality_tables(1)[0].max() == 255
    assert int(J.quality_tables(25)[0][0]) == (16 * 200 + 50) // 100
    if _turbo():
        src = np.zeros((8, 8, 3), dtype=np.uint8)
        for q in range(1, 101):
            for mode in ("4:2:0", "L"):
                head = J.header(8, 8, q, mode, 1)
                assert G.pillow_file(src, mode, q, 1).startswith(head), (q, mode)
    # the words the device reads come from the same objects as the header
    words, max_dc, max_ac = J.device_tables(75)
    assert words.shape == (J.TABLE_WORDS,) and (max_dc, max_ac) == (11, 16)
    assert np.array_equal(words[:64], J.quality_tables(75)[0]) and np.array_equal(words[64:128], J.quality_tables(75)[1])
    code, length = J.huffman_codes(J.AC_CHROMA)
    assert np.array_equal(words[160 + 256:] >> 16, length) and np.array_equal(words[160 + 256:] & 0xFFFF, code)
    # and their layout and the modes' numbers are the ones the library's header declares
    from ir2rgb_amd.jpeg_common import MODES
    with open(os.path.join(os.path.dirname(HERE), "include", "ir2rgb_hip.h")) as f:
        text = f.read()
    assert f"#define IR2RGB_JPEG_TABLE_WORDS {J.TABLE_WORDS}\n" in text
    for name, mode in (("444", "4:4:4"), ("420", "4:2:0"), ("L", "L"), ("422", "4:2:2")):
        assert f"#define IR2RGB_JPEG_{name} {MODES.index(mode)}\n" in text
    assert J.MODES == MODES[:3]


@pytest.mark.parametrize("fault", ["quant_floor", "chroma_bias_2", "chroma_pad_output", "dummy_real_dct", "no_stuffing",
                                   "no_predictor_reset"])
def test_equality_catches_planted_faults(goldens, fault, monkeypatch):
    monkeypatch.setattr(J, "_FAULTS", frozenset([fault]))
    caught = [m["name"] for m, src, want in goldens[0] if _reference(m, src)[0] != want]
    assert caught, f"no golden notices {fault}"
    monkeypatch.setattr(J, "_FAULTS", frozenset())
    m, src, want = goldens[0][0]
    assert _reference(m, src)[0] == want


def test_reference_refuses_bad_input():
    with pytest.raises(TypeError):
        J.jpeg_reference(np.zeros((8, 8, 3), dtype=np.float32))
    with pytest.raises(ValueError):
        J.jpeg_reference(np.zeros((8, 8, 2), dtype=np.uint8))
    with pytest.raises(ValueError):
        J.jpeg_reference(np.zeros((8, 8, 1), dtype=np.uint8), subsampling="4:2:0")
    with pytest.raises(ValueError):
        J.jpeg_reference(np.zeros((8, 8, 3), dtype=np.uint8), subsampling="4:2:2")
    with pytest.raises(ValueError):
        J.jpeg_reference(np.zeros((8, 8, 3), dtype=np.uint8), restart_rows=-1)
    with pytest.raises(ValueError, match="GPU only"):
        J.JpegEncoder("cpu", 8, 8)


def test_library_refuses_bad_arguments_before_any_launch():
    import torch
    from ir2rgb_amd import _lib, build
    build.build()
    lib = _lib.lib()
    H, W, hb = 17, 33, 623
    cap = lib.ir2rgb_jpeg_capacity_bytes(H, W, 1, 1, hb, 11, 16)
    ws = lib.ir2rgb_jpeg_workspace_bytes(2, H, W, 1, 1, 11, 16)
    # the derivation of include/ir2rgb_hip.h: 2 MCU rows of 3 MCUs of 6 blocks, (11 + 11) + 63 * 26 bits a block
    per_interval = (2 * ((18 * 1660 + 7) // 8) + 15) // 16 * 16
    assert cap == hb + 2 * (per_interval + 2)
    assert ws == 2 * 36 * 128 + 16 + 2 * 2 * per_interval
    assert lib.ir2rgb_jpeg_capacity_bytes(H, W, 1, 0, hb, 11, 16) == -1 and lib.ir2rgb_jpeg_capacity_bytes(H, W, 3, 1, hb, 11, 16) == -1
    assert lib.ir2rgb_jpeg_capacity_bytes(H, W, 1, 1, hb, 17, 16) == -1 and lib.ir2rgb_jpeg_workspace_bytes(0, H, W, 1, 1, 11, 16) == -1
    assert lib.ir2rgb_jpeg_workspace_bytes(1, 8, 65535, 2, 9, 11, 16) == -1          # an interval above 65535 MCUs
    p = torch.zeros(64).data_ptr()
    assert p % 16 == 0

    def call(src=p, out=p, lengths=p, wsp=p, ws_bytes=ws, header=p, header_bytes=hb, tables=p, N=2, C=3, mode=1, rr=1, capacity=cap):
        return lib.ir2rgb_jpeg_encode_u8(src, out, lengths, wsp, ws_bytes, header, header_bytes, tables, N, C, H, W, mode, rr, 11,
                                         16, capacity, None)

    for kw in (dict(src=None), dict(out=None), dict(lengths=None), dict(wsp=None), dict(header=None), dict(tables=None),
               dict(ws_bytes=ws - 1), dict(capacity=cap - 1), dict(rr=0), dict(rr=-3), dict(N=0), dict(C=1), dict(C=2), dict(mode=3),
               dict(header_bytes=0)):
        assert call(**kw) == -1, kw
    for kw in (dict(wsp=p + 8), dict(tables=p + 2), dict(lengths=p + 1)):
        assert call(**kw) == -3, kw
    with pytest.raises(ValueError, match="jpeg_capacity_bytes"):
        _lib.query("ir2rgb_jpeg_capacity_bytes", H, W, 1, 0, hb, 11, 16)
