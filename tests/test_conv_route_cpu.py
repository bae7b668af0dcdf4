"""The convolution dispatch of libir2rgb_hip.so, pinned without a GPU: tests/golden/conv_routes.json holds what the host
queries answered, for the descriptor list of tests/golden/make_route_goldens.py, before the dispatch code was last
reorganised.  The built library must answer every row exactly so: kernel name, statistics rows, packed-weight elements,
forward workspace, both weight-gradient workspaces, the weight gradient's argument check and the batched repack's tables.
"""
import hashlib
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SWITCHES = ("IR2RGB_CONV3X3P", "IR2RGB_CONV3X3P_SPLIT", "IR2RGB_CONV_DOT")


def _maker():
    spec = importlib.util.spec_from_file_location("make_route_goldens", os.path.join(GOLDEN, "make_route_goldens.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


M = _maker()


@pytest.fixture(scope="module")
def golden():
    with open(M.PATH) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def descs():
    return M.descriptors()


@pytest.fixture(scope="module")
def lib():
    from ir2rgb_amd import _lib, build
    build.build()
    return _lib.lib()


def test_every_row_has_its_descriptor(golden, descs):
    """The enumeration rebuilds exactly the recorded list: same length, same descriptors in the same order."""
    assert len(descs) == len(set(descs)) == golden["descriptors"] == len(golden["rows"])
    assert hashlib.sha1(json.dumps(descs).encode()).hexdigest() == golden["descriptors_sha1"]
    assert tuple(golden["names"]) == M.NAMES
    assert 2000 <= len(descs) <= 5000
    assert os.path.getsize(M.PATH) < os.path.getsize(os.path.join(os.path.dirname(GOLDEN), "window_geometries.json"))


def test_rows_cover_every_kernel_and_every_error(golden):
    rows = golden["rows"]
    assert {r[0] for r in rows} == set(range(len(M.NAMES)))                  # the seven names and the empty one
    codes = {v for r in rows for v in r[1:7] if v < 0}
    codes |= {v for p in golden["pack"] for v in p if isinstance(v, int)}
    assert codes == {-1, -2, -3}                                             # IR2RGB_EINVAL, _ENOSUP, _EALIGN
    assert any(r[3] > 0 for r in rows) and any(r[4] == 4 for r in rows)      # a split patch form; the unsplit nine-tap form
    kinds = {(len(p[0]) == 4 and p[0][1], len(p[1]) == 4 and p[1][1]) for p in golden["pack"] if not isinstance(p[0], int)}
    assert {(1, 1), (4, 4), (2, 2)} <= kinds                                 # one entry, and a class each of 2 x 2 and 2 x 1


def test_library_answers_every_row_as_recorded(lib, golden, descs):
    for v in SWITCHES:
        assert v not in os.environ, f"{v} changes the dispatch: the table holds the defaults"
    rows, packs = M.answers(lib, descs)
    wrong = [(d, r, g) for d, r, g in zip(descs, rows, golden["rows"]) if r[:7] != g[:7] or packs[r[7]] != golden["pack"][g[7]]]
    assert not wrong, (len(wrong), [dict(zip(M.DESC_FIELDS, d)) for d, _, _ in wrong[:3]], [(r, g) for _, r, g in wrong[:3]])
