"""CPU tests of ir2rgb_amd.thermal.agc_reference, the numpy definition of the thermal AGC that csrc/thermal_agc.hip is held
to at tolerance 0 (tests/test_agc_gpu.py).  Nothing outside the project defines this function, so it is pinned from a
second direction: hand-worked numbers, the textbook formulas in exact rational arithmetic, invariants of the recurrence,
and a second model of the definition (``model`` below, written another way) in which faults can be planted -- each
must move a compared value (output bytes, levels, or the state S) on the test clip."""
from fractions import Fraction

import numpy as np
import pytest

from ir2rgb_amd.thermal import LEVELS, agc_options, agc_reference


def make_clip(n=5, H=37, W=53, seed=0):
    """A drifting sinusoidal background near 7000 counts with noise, a block 2500 counts warmer, one pixel at 40000 and
    one at 65535."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    frames = np.empty((n, H, W), np.uint16)
    for t in range(n):
        f = 7000 + 40 * t + 300 * np.sin(xx / 9.0 + 0.3 * t) * np.cos(yy / 7.0) + rng.normal(0, 6, (H, W))
        f[H // 4:H // 4 + max(1, H // 5), W // 3:W // 3 + max(1, W // 4)] += 2500
        f = np.clip(np.rint(f), 0, 65535).astype(np.uint16)
        f[H // 2, W // 2] = 40000
        f[H - 1, W - 1] = 65535
        frames[t] = f
    return frames


def model(frames, mode, plateau, a_q, tail_ppm, fault=None):
    """The definition once more, level by level where agc_reference is vectorised, with optional planted faults.
    -> (u8 [N,H,W], levels [N,2], S, luts [N,65536])"""
    k = 65536 - a_q
    S = None
    outs, levels, luts = [], [], []
    for x in frames:
        idx = x.astype(np.int64)
        if fault == "signed":
            idx = np.maximum(x.view(np.int16).astype(np.int64), 0)
        h = np.zeros(LEVELS, np.int64)
        np.add.at(h, idx.ravel(), 1)
        clip = mode == "plateau" and fault not in ("no_clip", "clip_after")
        G = (np.where(h > plateau, plateau, h) if clip else h) * 65536
        if S is None and fault != "skip_init":
            S = G.copy()
        else:
            prod = (G - (0 if S is None else S)) * k
            step = np.sign(prod) * (np.abs(prod) // 65536) if fault == "trunc" else np.floor_divide(prod, 65536)
            S = (0 if S is None else S) + step
        if mode == "plateau" and fault == "clip_after":
            S = np.minimum(S, plateau * 65536)
        Sl = [int(s) for s in S]
        C, run = [], 0
        for s in Sl:
            run += s
            C.append(run)
        T = C[-1]
        half = 0 if fault == "floor" else 1
        if mode == "plateau":
            occ = [v for v in range(LEVELS) if Sl[v] > 0]
            a, b = occ[0], occ[-1]
            c0 = 0 if fault == "no_c0" else C[a]
            D = T - c0
            lut = [0 if D == 0 else (max(c - c0, 0) * 255 + half * (D // 2)) // D for c in C]
        else:
            a = next(v for v in range(LEVELS) if C[v] * 10 ** 6 > T * tail_ppm)
            b = next(v for v in range(LEVELS) if C[v] * 10 ** 6 >= T * (10 ** 6 - tail_ppm))
            Wd = b - a
            lut = [0 if Wd == 0 else min(max(((v - a) * 255 + half * (Wd // 2)) // Wd, 0), 255) for v in range(LEVELS)]
        lut = np.array(lut, np.int64)
        assert lut.min() >= 0 and lut.max() <= 255
        luts.append(lut)
        levels.append((a, b))
        outs.append(lut[idx].astype(np.uint8))
    return np.stack(outs), np.array(levels, np.int32), np.asarray(S, np.int64), np.stack(luts)


@pytest.fixture(scope="module")
def clip():
    return make_clip()


OPTS = {"plateau": dict(mode="plateau", plateau=None, damping=0.875, tail_ppm=10000),
        "linear": dict(mode="linear", plateau=None, damping=0.875, tail_ppm=10000)}


# The planted faults run at damping 0.9.  At the default 0.875 the blend weight is 2^13 and every S of the clip's five
# frames is a multiple of 2^(16 - 3 t) after t updates, so the shift of frames 1..4 drops only zero bits and a truncating
# shift cannot differ from a flooring one before the seventh frame.  0.9 is a_q = 58982, weight 6554: no power of two.
FAULT_OPTS = {mode: dict(o, damping=0.9) for mode, o in OPTS.items()}


@pytest.fixture(scope="module")
def clean(clip):
    """agc_reference and the fault-free model on the clip, per mode, at FAULT_OPTS (computed once)."""
    res = {}
    for mode, o in FAULT_OPTS.items():
        _, plateau, a_q, tail, _ = agc_options(clip[0].size, **o)
        res[mode] = (agc_reference(clip, channels=1, **o), model(clip, mode, plateau, a_q, tail))
    return res


def test_options_are_the_stated_integers():
    assert agc_options(512 * 640) == (0, 320, 57344, 10000, 3)
    assert agc_options(100, damping=0)[1:3] == (1, 0)
    assert agc_options(100, damping=65535 / 65536)[2] == 65535 and agc_options(100, damping=1 - 2.0 ** -30)[2] == 65535
    for bad in (dict(mode="clahe"), dict(plateau=0), dict(damping=1.0), dict(damping=-0.1), dict(tail_ppm=500000),
                dict(tail_ppm=-1), dict(channels=2)):
        with pytest.raises(ValueError):
            agc_options(100, **bad)
    with pytest.raises(TypeError):
        agc_reference(np.zeros((2, 2), np.uint8))
    with pytest.raises(ValueError):
        agc_reference(np.zeros((2, 2, 2, 2), np.uint16))


def test_hand_worked_frames_plateau():
    a = np.array([[100, 100, 100, 102], [102, 105, 105, 105]], np.uint16)
    b = np.full((2, 4), 102, np.uint16)
    # h = 3, 2, 3 at 100, 102, 105
    u8, levels, S = agc_reference(a, mode="plateau", plateau=2, damping=0.5, channels=1)
    # g = min(h, 2) = 2, 2, 2; S = g << 16; C = 131072, 262144, 393216 = T; c0 = 131072, D = 262144
    assert {v: int(S[v]) for v in np.flatnonzero(S)} == {100: 131072, 102: 131072, 105: 131072}
    assert levels.tolist() == [[100, 105]]
    # lut[102] = (131072 * 255 + 131072) // 262144 = 128; lut[105] = (262144 * 255 + 131072) // 262144 = 255
    assert u8[..., 0].tolist() == [[0, 0, 0, 128], [128, 255, 255, 255]]
    # frame b, damping 0.5 (k = 32768): h[102] = 8 -> g = 2, G = 131072
    #   S[100] = 131072 + ((0 - 131072) * 32768 >> 16) = 65536,  S[102] = 131072 + 0,  S[105] = 65536;  T = 262144
    #   c0 = 65536, D = 196608;  lut[102] = (131072 * 255 + 98304) // 196608 = 33521664 // 196608 = 170
    u8b, levels_b, Sb = agc_reference(np.stack([a, b]), mode="plateau", plateau=2, damping=0.5, channels=3)
    assert {v: int(Sb[v]) for v in np.flatnonzero(Sb)} == {100: 65536, 102: 131072, 105: 65536}
    assert levels_b.tolist() == [[100, 105], [100, 105]]
    assert u8b.shape == (2, 2, 4, 3) and (u8b[0] == u8).all() and (u8b[1] == 170).all()
    # the same continuation through state=
    u8c, _, Sc = agc_reference(b, mode="plateau", plateau=2, damping=0.5, channels=3, state=S)
    assert (u8c == u8b[1]).all() and (Sc == Sb).all()
    # unclipped (plateau = P): g = 3, 2, 3; C = 196608, 327680, 524288; c0 = 196608, D = 327680
    #   lut[102] = (131072 * 255 + 163840) // 327680 = 33587200 // 327680 = 102
    u8p, _, Sp = agc_reference(a, mode="plateau", plateau=8, damping=0.5, channels=1)
    assert [int(Sp[v]) for v in (100, 102, 105)] == [196608, 131072, 196608]
    assert u8p[..., 0].tolist() == [[0, 0, 0, 102], [102, 255, 255, 255]]


def test_hand_worked_frame_linear():
    a = np.array([[100, 100, 100, 102], [102, 105, 105, 105]], np.uint16)
    # S = h << 16 = 196608, 131072, 196608; C = 196608, 327680, 524288 = T
    # tail 20 %: lo: C 10^6 > T 200000 = 1.048576e11 -> first at 100;  hi: C 10^6 >= T 800000 = 4.194304e11 -> 105 (3.2768e11 < it)
    # Wd = 5: lut[102] = (2 * 255 + 2) // 5 = 102
    u8, levels, S = agc_reference(a, mode="linear", tail_ppm=200000, damping=0.5, channels=1)
    assert [int(S[v]) for v in (100, 102, 105)] == [196608, 131072, 196608] and int(S.sum()) == 524288
    assert levels.tolist() == [[100, 105]]
    assert u8[..., 0].tolist() == [[0, 0, 0, 102], [102, 255, 255, 255]]
    # tail 40 %: lo: > T 0.4 = 209715.2 -> 102 (C = 327680);  hi: >= T 0.6 = 314572.8 -> 102: Wd = 0, all zero
    u8z, levels_z, _ = agc_reference(a, mode="linear", tail_ppm=400000, damping=0.5, channels=1)
    assert levels_z.tolist() == [[102, 102]] and not u8z.any()


def test_plateau_P_without_damping_is_textbook_equalisation(clip):
    x = clip[0]
    P = x.size
    u8, levels, _ = agc_reference(x, mode="plateau", plateau=P, damping=0, channels=1)
    h = np.bincount(x.ravel(), minlength=LEVELS)
    cdf = np.cumsum(h)
    cdf_min = int(cdf[levels[0, 0]])
    assert cdf_min == int(h[x.min()]) and levels[0].tolist() == [int(x.min()), int(x.max())]
    want = {int(v): int(Fraction(255 * (int(cdf[v]) - cdf_min), P - cdf_min) + Fraction(1, 2)) for v in np.unique(x)}
    assert (u8[..., 0] == np.vectorize(want.get)(x)).all()


def test_linear_without_tails_is_min_max_stretch(clip):
    x = clip[0]
    u8, levels, _ = agc_reference(x, mode="linear", tail_ppm=0, damping=0, channels=1)
    lo, hi = int(x.min()), int(x.max())
    assert levels[0].tolist() == [lo, hi]
    want = {int(v): int(Fraction(255 * (int(v) - lo), hi - lo) + Fraction(1, 2)) for v in np.unique(x)}
    assert (u8[..., 0] == np.vectorize(want.get)(x)).all()


@pytest.mark.parametrize("mode", ["plateau", "linear"])
def test_reference_equals_the_second_model_and_luts_are_monotone(clean, clip, mode):
    (u8, levels, S), (m_u8, m_levels, m_S, luts) = clean[mode]
    assert (u8[..., 0] == m_u8).all() and (levels == m_levels).all() and (S == m_S).all()
    assert (np.diff(luts, axis=1) >= 0).all() and luts.min() >= 0 and luts.max() <= 255
    if mode == "plateau":
        for lut, (v0, v1) in zip(luts, levels):
            assert lut[v0] == 0 and lut[v1] == 255         # D > 0 on the clip: more than one level is occupied
    u3 = agc_reference(clip, channels=3, **FAULT_OPTS[mode])[0]
    assert u3.shape == (*clip.shape, 3) and (u3 == u8).all()


FAULTS = {"plateau": ["no_clip", "clip_after", "no_c0", "floor", "signed", "trunc", "skip_init"],
          "linear": ["floor", "signed", "trunc", "skip_init"]}


@pytest.mark.parametrize("mode,fault", [(m, f) for m, fs in FAULTS.items() for f in fs])
def test_planted_faults_move_a_compared_value(clean, clip, mode, fault):
    _, plateau, a_q, tail, _ = agc_options(clip[0].size, **FAULT_OPTS[mode])
    (u8, levels, S), _ = clean[mode]
    f_u8, f_levels, f_S, _ = model(clip, mode, plateau, a_q, tail, fault=fault)
    moved = {"bytes": bool((f_u8 != u8[..., 0]).any()), "levels": bool((f_levels != levels).any()), "S": bool((f_S != S).any())}
    assert any(moved.values()), fault
    if fault == "trunc":
        assert moved["S"]                   # a one-LSB error in Q16: only the state is sure to show it
    elif fault != "skip_init":
        assert moved["bytes"], (fault, moved)


@pytest.mark.parametrize("mode", ["plateau", "linear"])
def test_constant_sequence_is_a_fixed_point(clip, mode):
    seq = np.repeat(clip[:1], 4, axis=0)
    u8, levels, S = agc_reference(seq, channels=1, **OPTS[mode])
    u1, l1, S1 = agc_reference(clip[0], channels=1, **OPTS[mode])
    assert (u8 == u1[None]).all() and (levels == l1).all() and (S == S1).all()


@pytest.mark.parametrize("mode", ["plateau", "linear"])
def test_without_damping_every_frame_stands_alone(clip, mode):
    o = dict(OPTS[mode], damping=0)
    u8, levels, S = agc_reference(clip, channels=1, **o)
    for t in range(len(clip)):
        ut, lt, St = agc_reference(clip[t], channels=1, **o)
        assert (u8[t] == ut).all() and (levels[t] == lt[0]).all()
    assert (S == St).all()


@pytest.mark.parametrize("mode", ["plateau", "linear"])
def test_state_stays_bounded_at_the_largest_damping(mode):
    frames = make_clip(40, 16, 24, seed=3)
    P = frames[0].size
    o = dict(OPTS[mode], damping=65535 / 65536)
    S = None
    for t in range(40):
        _, _, S = agc_reference(frames[t], channels=1, state=S, **o)
        assert S.min() >= 0 and 0 < int(S.sum()) <= P << 16, t
    whole = agc_reference(frames, channels=1, **o)[2]
    assert (whole == S).all()


@pytest.mark.parametrize("mode", ["plateau", "linear"])
@pytest.mark.parametrize("frame", [np.array([[1234]], np.uint16), np.zeros((3, 5), np.uint16), np.full((3, 5), 65535, np.uint16)],
                         ids=["1x1", "all0", "all65535"])
def test_degenerate_frames_give_zero(mode, frame):
    with np.errstate(all="raise"):
        u8, levels, S = agc_reference(np.stack([frame, frame]), channels=3, **OPTS[mode])
    assert not u8.any() and (levels == int(frame[0, 0])).all() and np.count_nonzero(S) == 1


def test_int16_input_is_reinterpreted_as_unsigned(clip):
    a = agc_reference(clip, **OPTS["plateau"])
    b = agc_reference(clip.view(np.int16), **OPTS["plateau"])
    assert all((p == q).all() for p, q in zip(a, b))
