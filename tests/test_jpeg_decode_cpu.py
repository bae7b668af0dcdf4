"""The JPEG decoder's definition (ir2rgb_amd/jpeg_decode.py) on the host: ``decode_reference`` against files written and
decoded by Pillow (tests/golden/jpeg_decode_cases.npz, tolerance 0; against a live Pillow too where it imports), ``parse``,
the parallel entropy decode ``entropy_model`` against the sequential decoder, planted faults, the liveness of the cases,
``frames.video_params`` against the reference's recorded draws and ``frames.FolderSequences``' ordering.  No GPU."""
import hashlib
import io
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
import make_jpeg_decode_goldens as G  # noqa: E402

from ir2rgb_amd import jpeg_decode as D  # noqa: E402
from ir2rgb_amd.jpeg import jpeg_reference  # noqa: E402


@pytest.fixture(scope="module")
def goldens():
    return G.load()


@pytest.fixture(scope="module")
def cases(goldens):
    return goldens[0]


def test_the_cases_are_the_ones_the_issue_names(cases):
    names = {m["name"] for m, _, _ in cases}
    assert len(cases) == 196
    for h, w in G.SHAPES:
        for mode in G.MODES:
            for q in G.QUALITIES:
                assert f"{h}x{w}/{mode}/q{q}" in names
    assert {-(-m["hw"][1] // 2) for m, _, _ in cases if m["mode"] in ("4:2:0", "4:2:2")} >= {1, 2, 3}
    assert {m["restart_rows"] for m, _, _ in cases} == {0, 1, 2} and any(m["optimize"] for m, _, _ in cases)
    assert {m["content"] for m, _, _ in cases} == set(G.CONTENTS)
    assert max(len(D.parse(d).segments) for _, d, _ in cases) > 9        # the marker number wraps


def test_decode_reference_equals_pillow_on_every_golden(cases):
    for m, data, want in cases:
        got = D.decode_reference(data)
        assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want), m["name"]


def test_full_size_files_equal_pillow(goldens):
    for m, data in goldens[1]:
        got = D.decode_reference(data)
        assert list(got.shape) == m["shape"] and hashlib.sha256(got.tobytes()).hexdigest() == m["sha256"], m["mode"]


def test_decode_reference_equals_a_live_pillow(cases):
    Image = pytest.importorskip("PIL.Image")
    for m, data, want in cases[::7]:
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(data))), D.decode_reference(data)), m["name"]
    exif = cases[40][1]
    exif = exif[:2] + b"\xff\xe1\x00\x10Exif\x00\x00" + bytes(8) + exif[2:]       # an application segment is skipped
    assert np.array_equal(D.decode_reference(exif), cases[40][2])
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(exif))), cases[40][2])


def _patched(data, old, new, count=1):
    assert data.count(old) >= 1, old
    return data.replace(old, new, count)


def test_parse_reads_the_header_and_tiles_the_scan(cases):
    for m, data, _ in cases:
        info = D.parse(data)
        assert (info.H, info.W, info.mode) == (*m["hw"], m["mode"])
        g = info.geometry
        assert data[info.scan[1]:info.scan[1] + 2] == b"\xff\xd9" and info.scan[1] + 2 == len(data)
        pos, mcu = info.scan[0], 0
        for k, s in enumerate(info.segments):
            assert (s.begin, s.first_mcu) == (pos, mcu) and s.n_mcus > 0
            if k + 1 < len(info.segments):
                assert data[s.end:s.end + 2] == bytes([0xFF, 0xD0 + (k & 7)])
            pos, mcu = s.end + 2, mcu + s.n_mcus
        assert pos == info.scan[1] + 2 and mcu == g.n_mcus
        rows = m["restart_rows"]
        assert len(info.segments) == (-(-g.mcu_rows // rows) if rows else 1)
        assert info.restart_interval == rows * g.mcus_per_row


def test_parse_rejects_what_it_does_not_support(cases):
    by = {m["name"]: d for m, d, _ in cases}
    colour, grey = by["17x33/4:2:0/q75"], by["17x33/L/q75"]
    sof = colour.index(b"\xff\xc0")
    dqt = colour.index(b"\xff\xdb")
    sos = colour.index(b"\xff\xda")

    def with_byte(d, at, value):
        return d[:at] + bytes([value]) + d[at + 1:]

    unsupported = [
        (with_byte(colour, sof + 1, 0xC2), "progressive"),
        (with_byte(colour, sof + 1, 0xC9), "arithmetic"),
        (with_byte(colour, sof + 1, 0xC1), "extended"),
        (with_byte(colour, sof + 4, 12), "12-bit"),
        (with_byte(colour, sof + 9, 4), "4 components"),
        (with_byte(colour, sof + 11, 0x41), "sampling factors"),
        (with_byte(colour, sof + 14, 0x21), "sampling factors"),
        (with_byte(colour, dqt + 4, 0x10), "16-bit quantisation"),
        (with_byte(colour, sos + 4, 1), "scan of 1 of 3"),
        (with_byte(colour, sos + 6, 0x22), "Huffman table id"),
        (with_byte(colour, sos + len(colour[sos:sos + 4]) + 8, 5), "progressive"),
        (_patched(colour, b"JFIF\x00", b"JFXX\x00").replace(b"\x01\x22\x00\x02\x11\x01\x03\x11\x01", b"R\x22\x00G\x11\x01B\x11\x01")
         .replace(b"\x03\x01\x00\x02\x11\x03\x11", b"\x03R\x00G\x11B\x11"), "RGB-coded"),
        (colour[:-2] + colour[sos:], "several scans"),
    ]
    for data, what in unsupported:
        with pytest.raises(NotImplementedError, match=what):
            D.parse(data)
    malformed = [colour[:sof + 6], colour[:sos + 3], colour[:dqt + 30], b"\x89PNG\r\n\x1a\n" + bytes(16), colour[:2], b"",
                 with_byte(colour, sof + 3, 9), colour[:2] + b"\xff\xd9", colour[:sof] + colour[sos:]]
    for data in malformed:
        with pytest.raises(ValueError):
            D.parse(data)
    assert D.parse(grey).mode == "L" and D.parse(colour).mode == "4:2:0"
    # a damaged scan is the decoder's business, not parse's
    with pytest.raises(ValueError, match="damaged scan"):
        D.decode_reference(colour[:len(colour) - 40] + b"\xff\xd9")


def test_entropy_model_reaches_the_sequential_states(cases):
    worst = 0
    for m, data, _ in cases[::7] + [c for c in cases if c[0]["name"].startswith(("long/4:2:0", "tall/"))]:
        info = D.parse(data)
        longest = max(s.end - s.begin for s in info.segments)
        for sub in (4, 16, 64, 256, longest + 1):
            for seg, rec in zip(info.segments, D.entropy_model(info, sub)):
                assert rec["status"] == 0 and rec["rounds"] <= rec["n_sub"] <= D.ENT_THREADS, (m["name"], sub)
                assert rec["sub_bytes"] == D.effective_sub_bytes(seg.end - seg.begin, sub)
                assert rec["entries"] == D.sequential_states(info, seg, sub), (m["name"], sub)
                worst = max(worst, rec["rounds"])
            if sub > longest:
                assert all(r["n_sub"] == 1 and r["rounds"] == 1 for r in D.entropy_model(info, sub))
    assert worst > 4                # the many-rounds path


def test_entropy_model_writes_the_sequential_coefficients(cases):
    for m, data, _ in cases[5::16]:
        info = D.parse(data)
        g = info.geometry
        want = D.scan_coefficients(info)
        for sub in (4, 64):
            for seg, rec in zip(info.segments, D.entropy_model(info, sub, coefficients=True)):
                blocks = rec["blocks"].astype(np.int64)
                for c in range(g.ncomp):                # the DC is still a difference: sum it per component
                    rows = [b for b in range(len(blocks)) if g.comp_of[b % g.blocks_per_mcu] == c]
                    blocks[rows, 0] = np.cumsum(blocks[rows, 0])
                lo = seg.first_mcu * g.blocks_per_mcu
                assert np.array_equal(blocks, want[lo:lo + len(blocks)]), (m["name"], sub)


@pytest.mark.parametrize("fault", ["fancy_narrow", "bias_swapped", "far_row_top", "no_predictor_reset", "dc_across_components",
                                   "fix_floor", "no_unstuffing"])
def test_a_planted_fault_changes_a_golden(cases, fault, monkeypatch):
    monkeypatch.setattr(D, "_FAULTS", frozenset([fault]))
    changed = 0
    for m, data, want in cases:
        try:
            got = D.decode_reference(data)
        except ValueError:
            changed += 1
            continue
        changed += not np.array_equal(got, want)
    assert changed > 0, fault


def test_the_cases_reach_every_rule(cases):
    cnt = G.liveness(cases[::5] + [c for c in cases if c[0]["name"].startswith(("long/L", "tall/4:4:4", "flat/"))])
    assert set(cnt) == set(D.COUNTERS)
    dead = [k for k, v in cnt.items() if not v]
    assert not dead, f"the cases never reach: {dead}"


def test_video_params_equals_the_reference_draws():
    from ir2rgb_amd.frames import video_params
    with open(G.PARAMS) as f:
        records = json.load(f)["records"]
    assert len(records) == 160
    for r in records:
        opt = {k: v for k, v in r["opt"].items() if k != "debug"}
        got = video_params(r["seq_len"], 0, rng=np.random.RandomState(r["seed"]), **opt)
        assert list(got) == r["result"], r
    np.random.seed(records[7]["seed"])          # the default source is numpy.random, as in the reference
    assert list(video_params(records[7]["seq_len"], 0, **{k: v for k, v in records[7]["opt"].items() if k != "debug"})) == records[7]["result"]
    assert video_params(30, 5, n_frames_total=6, n_input_gen_frames=3, is_train=False) == (3, 5, 1)


def _tree(root, layout):
    rng = np.random.default_rng(3)
    for folder, n in layout.items():
        os.makedirs(os.path.join(root, folder))
        grey = "lwir" in folder
        frames = rng.integers(0, 256, (n, 16, 24, 1 if grey else 3), dtype=np.uint8)
        for k, data in enumerate(jpeg_reference(frames, 75, "L" if grey else "4:2:0", 0)):
            with open(os.path.join(root, folder, "I%05d.jpg" % (n - k)), "wb") as f:      # written out of order
                f.write(data)


def test_folder_sequences_order_pair_and_check(tmp_path):
    from ir2rgb_amd.frames import FolderSequences, grouped_files
    good = str(tmp_path / "good")
    _tree(good, {"set01/V000/lwir": 3, "set01/V000/visible": 3, "set00/V001/lwir": 5, "set00/V001/visible": 5,
                 "set00/V000/lwir": 4, "set00/V000/visible": 4})
    groups = grouped_files(good)
    assert [os.path.relpath(os.path.dirname(g[0]), good) for g in groups] == [
        "set00/V000/lwir", "set00/V000/visible", "set00/V001/lwir", "set00/V001/visible", "set01/V000/lwir", "set01/V000/visible"]
    assert all(g == sorted(g) for g in groups)
    seqs = FolderSequences("cpu", good)
    assert len(seqs) == 3 and seqs.seq_len_max == 5 and [len(p) for p in seqs.ir_paths] == [4, 5, 3]
    for a, b in zip(seqs.ir_paths, seqs.rgb_paths):
        assert [p.replace("lwir", "visible") for p in a] == b
    short = str(tmp_path / "short")
    _tree(short, {"V000/lwir": 3, "V000/visible": 2})
    with pytest.raises(ValueError, match="3 frames"):
        FolderSequences("cpu", short)
    lone = str(tmp_path / "lone")
    _tree(lone, {"V000/lwir": 2, "V000/visible": 2, "V001/lwir": 2})
    with pytest.raises(ValueError, match="2 lwir and 1 visible"):
        FolderSequences("cpu", lone)
    png = str(tmp_path / "png")
    _tree(png, {"V000/lwir": 2, "V000/visible": 2})
    os.rename(os.path.join(png, "V000/lwir/I00001.jpg"), os.path.join(png, "V000/lwir/I00001.png"))
    with pytest.raises(ValueError, match="I00001.png"):
        FolderSequences("cpu", png)
    with pytest.raises(ValueError):
        FolderSequences("cpu", str(tmp_path / "nowhere"))


def test_malformed_inputs_report_through_the_model(cases):
    """The inputs of the GPU ``malformed`` step: the model returns, and names the damage."""
    from test_jpeg_decode_gpu import _malformed
    parsed = [(m, D.parse(d), w) for m, d, w in cases]
    seen = 0
    found = _malformed(parsed)
    assert len(found) >= 12
    for name, info in found:
        status = 0
        for sub in (D.DEFAULT_SUB_BYTES, 16):
            recs = D.entropy_model(info, sub)
            st = 0
            for r in recs:
                st |= r["status"]
                assert r["rounds"] <= max(r["n_sub"], 0) or r["n_sub"] == 0
            status = status or st
            assert st == status, name               # the status does not depend on sub_bytes
        assert status != 0, name
        if "truncated" in name:
            assert status & D.ERR_BLOCKS, name
        if "last record" in name:
            assert status == D.ERR_SEGMENT, name
        if "first record" in name:
            assert status & D.ERR_BLOCKS, name
        seen |= status
    assert seen & D.ERR_BLOCKS and seen & D.ERR_SEGMENT


def test_device_tables_are_what_the_header_documents(cases):
    info = D.parse(cases[60][1])
    t = D.device_tables(info)
    assert t.dtype == np.int32 and t.shape == (D.TABLE_WORDS,)
    with open(os.path.join(os.path.dirname(HERE), "include", "ir2rgb_hip.h")) as f:
        text = f.read()
    assert f"#define IR2RGB_JPEGD_TABLE_WORDS {D.TABLE_WORDS}" in text and f"#define IR2RGB_JPEGD_THREADS {D.ENT_THREADS}" in text
    assert f"#define IR2RGB_JPEG_422 {D.MODES.index('4:2:2')}" in text
    for name, bit in (("ECODE", D.ERR_CODE), ("EINDEX", D.ERR_INDEX), ("EBLOCKS", D.ERR_BLOCKS), ("ELEFTOVER", D.ERR_LEFTOVER),
                      ("ESEGMENT", D.ERR_SEGMENT)):
        assert f"#define IR2RGB_JPEGD_{name} {bit} " in text
    # every code of every table decodes to its symbol through limit / offset / values
    for (cls, tid), (bits, vals) in info.huffman.items():
        limit, offset, values = D.huffman_decode_table((bits, vals))
        code, k = 0, 0
        for n in range(1, 17):
            for _ in range(bits[n - 1]):
                w = code << (16 - n)
                length = next(l for l in range(1, 17) if w < limit[l - 1])
                assert length == n and values[offset[n - 1] + (w >> (16 - n))] == vals[k]
                code, k = code + 1, k + 1
            code <<= 1


def test_public_names():
    import ir2rgb_amd
    assert ir2rgb_amd.JpegDecoder is D.JpegDecoder and ir2rgb_amd.decode_reference is D.decode_reference
    from ir2rgb_amd.frames import FolderSequences
    assert ir2rgb_amd.FolderSequences is FolderSequences
    with pytest.raises(ValueError, match="AMD GPU only"):
        D.JpegDecoder("cpu", 8, 8, "L")
