"""The range-aware oracle (oracle.bounds.check_range, oracle/range_cases.py) without a GPU.

(a) every EDGE_RANGE record is live in each of its modes, judged from the fp64 reference alone: an overflow case
    demands inf of >= 10 % and finite of >= 10 % of its outputs with <= 2 % undecided, a subnormal case has >= 25 % of
    its half outputs in [2^-23, 2^-15), a nonfinite case has a footprint that is neither empty nor everything;
(b) in the manner of tests/test_kernel_bounds_cpu.py: the fp64 result rounded to the output format passes, and each of
    five wrong stores, emulated on that rounded result, is rejected on every case it applies to -- saturating at 65504,
    rounding toward zero at the top of f16's range, flushing f16 subnormals, ``x > 0 ? x : 0`` on a NaN, dropping the
    sign of an inf;
(c) today's oracle.bounds.check accepts the flushing store: why the new check exists.
"""
import math

import numpy as np
import pytest

from oracle import bounds as B
from oracle import range_cases as RC
from oracle import window as WG
from oracle.edge_records import EDGE_RANGE, RANGE_CASES
from oracle.replay import rnd

IDS = [f"{WG.launch_id(r)}-{m}-{(r.get('plant') or ('',))[0]}" for r, m in RANGE_CASES]
F16_MAX = 65504.0


# the five wrong stores, on the rounded result ``v`` of the reference ``ref`` (what a faultless kernel stores)
def saturating(v, ref, fmt):
    return np.where(np.isinf(v) & np.isfinite(ref), np.sign(v) * F16_MAX, v) if fmt == "f16" else v


def toward_zero_at_the_top(v, ref, fmt):
    with np.errstate(invalid="ignore"):
        top = np.isfinite(ref) & (np.abs(ref) > F16_MAX) & (np.abs(ref) < 65536.0)
    return np.where(top, np.sign(ref) * F16_MAX, v) if fmt == "f16" else v


def flushing(v, ref, fmt):
    with np.errstate(invalid="ignore"):
        return np.where(np.abs(v) < 2.0 ** -14, 0.0, v) if fmt == "f16" else v


def nan_to_zero(v, ref, fmt):
    """``x > 0 ? x : 0`` where the value is NaN (the finite and infinite elements keep their values)."""
    return np.where(np.isnan(v), 0.0, v)


def unsigned_inf(v, ref, fmt):
    return np.where(np.isinf(v), math.inf, v)


FAULTS = {"saturating": saturating, "toward_zero_at_the_top": toward_zero_at_the_top, "flushing": flushing,
          "nan_to_zero": nan_to_zero, "unsigned_inf": unsigned_inf}


def _applies(name, o, v):
    """Whether the fault changes an element of ``o`` whose value check_range pins (oracle.bounds.range_masks)."""
    ref, fmt = o["ref"], o["fmt"]
    with np.errstate(all="ignore"):
        fin, bnd, must_inf, _ = B.range_masks(ref, o["acc"], fmt)
        a = np.where(fin, np.abs(ref), 0.0)
        if name == "saturating":
            return bool(must_inf.any())
        if name == "toward_zero_at_the_top":
            return bool((must_inf & (a < 65536.0)).any())
        if name == "flushing":
            return fmt == "f16" and bool((fin & (a < 2.0 ** -14) & (a > bnd)).any())
        if name == "nan_to_zero":
            return bool(np.isnan(ref).any())
        return bool((must_inf & (ref < 0)).any() or (ref == -math.inf).any())


def _never_negative(rec):
    """Overflow cases without a negative overflow: a ReLU in front of the store and nothing added behind it."""
    if rec["entry"] == "ir2rgb_nchw_f32_to_nhwc_half_slice":      # act 2: LeakyReLU(0.1) holds N(0, 1) * 2^16 * 0.1 below 65520
        return rec["args"][8] == 2
    return rec["kind"] == "bn" and rec["entry"] != "ir2rgb_bn_bwd" and RC._bn_shape(rec)[2] == 1 and \
        not any(rec["args"][3:5] if rec["entry"] == "ir2rgb_bn_apply" else rec["args"][17:19])


@pytest.mark.parametrize("rec,mode", RANGE_CASES, ids=IDS)
def test_case_is_live_and_faulty_stores_are_rejected(rec, mode):
    expected = {"overflow": {"saturating"} if _never_negative(rec) else {"saturating", "unsigned_inf"}, "subnormal": set(),
                "nonfinite": set()}[mode]
    if mode == "nonfinite" and rec["kind"] != "op":
        expected = {"nan": {"nan_to_zero"}, "-inf": {"unsigned_inf"}, "+inf": set()}[rec["plant"][2]]
    for fmt in RC.MODE_FMTS[mode]:
        case = RC.build_for(rec)(rec, mode, fmt)
        ok, text = RC.liveness(case, mode)
        print(fmt, mode, text, case.get("note"))
        assert ok, f"{fmt}: not live: {text}"
        if mode == "subnormal" and any(o["fmt"] == "f16" for o in case["outs"]):
            expected = {"flushing"}
        applied = set()
        for o in case["outs"]:
            v = rnd(o["ref"], o["fmt"])
            ok, ratio, i, cnt = RC.check_out(o, v)
            assert ok, f"{fmt} {o['name']}: the rounded fp64 result fails at {np.unravel_index(i, v.shape)} ({cnt})"
            assert ratio <= 1.0
            for name, fault in FAULTS.items():
                if _applies(name, o, v):
                    applied.add(name)
                    bad = fault(v, o["ref"], o["fmt"])
                    assert not RC.check_out(o, bad)[0], f"{fmt} {o['name']}: the {name} store passes"
        assert expected <= applied, f"{fmt}: {sorted(expected - applied)} found nothing to break in this case"


def test_every_fault_meets_a_case():
    """toward_zero_at_the_top needs an output inside (65520 + its accumulation term, 65536), 16 wide: the converters'
    overflow inputs hold 65521 (convert_case), the other cases meet it by chance."""
    rec = next(r for r in EDGE_RANGE if r["entry"] == "ir2rgb_nchw_f32_to_nhwc_half")
    o = RC.convert_case(rec, "overflow", "f16")["outs"][0]
    v = rnd(o["ref"], "f16")
    assert _applies("toward_zero_at_the_top", o, v)
    assert not RC.check_out(o, toward_zero_at_the_top(v, o["ref"], "f16"))[0]


def test_threshold_of_the_overflow_check():
    """65519 -> 65504 is legal and 65521 -> 65504 is not; 65521 -> inf is legal, -65521 -> +inf is not."""
    def ok(got, ref, fmt="f16"):
        return B.check_range(np.array([got]), np.array([ref]), 0.0, fmt)[0]
    assert ok(65504.0, 65519.0) and not ok(math.inf, 65519.0)
    assert ok(math.inf, 65521.0) and not ok(65504.0, 65521.0)
    assert ok(-math.inf, -65521.0) and not ok(math.inf, -65521.0)
    assert ok(65504.0, 65520.0) and ok(math.inf, 65520.0)              # the midpoint itself: undecided
    assert B.check_range(np.array([65504.0]), np.array([65520.0]), 0.0, "f16")[3]["undecided"] == 1
    # subnormals: 2^-24 must survive, 2^-25 (the midpoint to zero) may go either way, both as exact values
    assert ok(2.0 ** -24, 2.0 ** -24) and not ok(0.0, 1.5 * 2.0 ** -24)
    assert ok(0.0, 2.0 ** -25) and ok(2.0 ** -24, 2.0 ** -25)
    # planted values: NaN wants anything non-finite, an inf that inf or NaN
    assert ok(math.nan, math.nan) and ok(math.inf, math.nan) and not ok(0.0, math.nan)
    assert ok(math.inf, math.inf) and ok(math.nan, math.inf) and not ok(-math.inf, math.inf) and not ok(65504.0, math.inf)
    # a finite reference refuses a non-finite result unless the record allows the element
    assert not ok(math.nan, 1.0)
    assert B.check_range(np.array([math.nan]), np.array([1.0]), 0.0, "f16", allow=np.array([True]))[0]
    # bf16 / f32 keep ETA and have no overflow threshold here
    assert ok(0.0, 2.0 ** -127, "bf16") and ok(70000.0, 70000.0, "f32") and not ok(math.inf, 70000.0, "f32")


def test_todays_check_accepts_the_flushing_store():
    """oracle.bounds.check has ETA = 2^-14 for f16: a kernel that flushed every subnormal output would pass it."""
    rec = next(r for r in EDGE_RANGE if r["kind"] == "conv" and r.get("form") == "store:vector")
    case = RC.forward_case(rec, "subnormal", "f16")
    o = case["outs"][0]
    flushed = flushing(rnd(o["ref"], "f16"), o["ref"], "f16")
    assert (flushed == 0).mean() > 0.9
    S = o["acc"] / B.b_rw(B.chain_fwd(rec["desc"]))
    assert B.check(flushed, o["ref"], S, "f16", B.chain_fwd(rec["desc"]))[0]
    assert not B.check_range(flushed, o["ref"], o["acc"], "f16")[0]
