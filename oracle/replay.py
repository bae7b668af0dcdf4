"""What the fp64 replay harnesses share (test-only): oracle/replay_ops.py for the non-convolution entry points,
oracle/replay_kernels.py for the convolutions and BatchNorm.

A replay takes a record in the format of tests/window_geometries.json -- a launch of the training window
(oracle/window.py) or a hand-written one (oracle/edge_records.py) -- draws its operands from a generator seeded by the
record, launches the entry point, compares every element with an fp64 reference under a bound of oracle/bounds.py and
returns the worst err/bound ratio per number format.  Nothing here loads the library before a launch asks for it.
"""
import hashlib
import time
import zlib

import numpy as np
import torch

from oracle import bounds as B
from oracle import window as WG

DTYPES = (("bf16", torch.bfloat16, 1), ("f16", torch.float16, 2))


def ids(recs):
    seen, out = {}, []
    for r in recs:
        i = WG.launch_id(r)
        seen[i] = seen.get(i, 0) + 1
        out.append(i if seen[i] == 1 else f"{i}#{seen[i]}")
    return out


def gen(rec):
    """The record's generator: seeded by a crc of the whole record, so a ``seed`` key in it changes the inputs."""
    return torch.Generator().manual_seed(zlib.crc32(WG.canon(rec).encode()))


RECORDER = None     # off unless digests() below installs one


def hand(role, name, t):
    """The one point a replay passes when it hands an operand to a launch (role "in") or a device output to its check
    ("out"): RECORDER(role, name, t) if a recorder is installed.  -> t"""
    if RECORDER is not None:
        RECORDER(role, name, t)
    return t


def digests(fn, *a):
    """fn(*a) (a replay of one record) under a recorder -> {"in": sha1 of the bytes of every operand handed in, in order,
    "out": [[name, sha1 of the bytes of that output], ...] in the order the outputs were checked}.  The names carry the
    number format.  tests/test_pointwise_bits_gpu.py holds the kernels to a table of these, bit for bit."""
    global RECORDER
    h_in, out = hashlib.sha1(), []

    def rec(role, name, t):
        raw = t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()
        if role == "in":
            h_in.update(f"{name} {tuple(t.shape)} {t.dtype};".encode() + raw)
        else:
            out.append([name, hashlib.sha1(raw).hexdigest()])
    assert RECORDER is None
    RECORDER = rec
    try:
        fn(*a)
    finally:
        RECORDER = None
    return {"in": h_in.hexdigest(), "out": out}


def call(entry, *a):
    from ir2rgb_amd import _lib
    ref = next(x for x in a if isinstance(x, torch.Tensor))
    for i, x in enumerate(a):
        if isinstance(x, torch.Tensor):
            hand("in", f"{entry} argument {i}", x)
    rc = getattr(_lib.lib(), entry)(*a, _lib.current_stream(ref))
    _lib.check(rc, entry)


def np64(t):
    return t.detach().double().cpu().numpy()


def assert_bound(name, ok, ratio, i, over, shape):
    assert ok, f"{name}: {over} elements over the bound (worst {ratio:.3g} at {np.unravel_index(i, shape)})"
    return ratio


def bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def differs(g, want):
    """Mask of the elements of two CPU tensors of one format whose bits differ.  The sign of a zero is not checked, nor
    the payload of a NaN where the reference is NaN too (oracle/range_cases.py plants them; no other reference has one)."""
    return (bits(g) != bits(want)) & ~((g == 0) & (want == 0)) & ~(torch.isnan(g) & torch.isnan(want))


def exact(name, got, ref_t):
    """got (device half / fp32) == the fp64 reference rounded to nearest even into got's format, bit for bit."""
    want = ref_t.to(got.dtype)
    g = hand("out", name, got).cpu()
    bad = differs(g, want)
    assert not bool(bad.any()), f"{name}: {int(bad.sum())} elements differ from the rounded fp64 result " \
                                f"(first at {tuple(int(v) for v in bad.nonzero()[0])})"
    return 0.0


def sentinel(shape, dtype, dev):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


def rnd(x, fmt):
    """An fp64 array rounded to a number format: what a faultless kernel would store (the CPU fault tests)."""
    dt = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[fmt]
    return torch.from_numpy(np.ascontiguousarray(x)).to(dt).double().numpy()


def passes(got, ref, bnd):
    return B.check_bound(got, ref, bnd)[0]


class Table:
    """The (launch id, worst err/bound per format, seconds) rows of one GPU test module, printed by its teardown_module
    (run with -s).  A family is the part of the launch id before the first "-": the entry point."""

    def __init__(self):
        self.rows = []

    def run(self, name, fn, *a, kernel=None):
        """Times fn(*a) -> {format: ratio}; keys that start with "stats" are the ratios of a convolution's statistics rows."""
        t0 = time.perf_counter()
        worst = fn(*a)
        dt = time.perf_counter() - t0
        self.rows.append((name, worst, dt, kernel))
        print(f"\n{name}{' ' + kernel if kernel else ''}: worst err/bound "
              + " ".join(f"{k} {v:.3f}" for k, v in worst.items()) + f" ({dt:.2f} s)")

    def report(self, title=None):
        """Every launch and the maxima per family; with a title, the maxima and the time only."""
        if not self.rows:
            return
        fam = {}
        for name, worst, _, _ in self.rows:
            f = name.split("-")[0]
            fam[f] = max(fam.get(f, 0.0), max(worst.values()))
        fams = ", ".join(f"{k} {v:.4f}" for k, v in sorted(fam.items()))
        secs = [t for _, _, t, _ in self.rows]
        if title:
            print(f"\n{title}, worst err/bound per family: " + fams)
            print(f"{title}: {len(secs)} launches, {sum(secs):.1f} s, slowest {max(secs):.2f} s")
            return
        kernels = any(k for _, _, _, k in self.rows)
        print("\nper-launch worst err/bound" + (" (bf16, f16):" if kernels else ":"))
        for name, worst, t, kern in self.rows:
            if kernels:
                stats = "".join(f" {k} {v:.3f}" for k, v in worst.items() if k.startswith("stats"))
                print(f"  {worst['bf16']:7.4f} {worst['f16']:7.4f}  {t:6.1f} s  {kern:28s} {name}{stats}")
            else:
                print("  " + " ".join(f"{k} {v:7.4f}" for k, v in worst.items()) + f"  {t:6.1f} s  {name}")
        print("per family: " + fams)


class RangeTable:
    """The rows of tests/test_range_gpu.py: per launch and mode the worst err/bound per format and check_range's four
    counts (must-inf, must-finite, undecided, non-finite reference elements), printed by its teardown_module (run with -s)."""

    def __init__(self):
        self.rows = []

    def run(self, name, mode, fn, *a, **kw):
        t0 = time.perf_counter()
        worst = fn(*a, mode=mode, **kw)
        dt = time.perf_counter() - t0
        counts = worst.pop("counts")
        self.rows.append((name, mode, worst, counts, dt))
        print(f"\n{name} [{mode}]: worst err/bound " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()) + f" ({dt:.2f} s)")

    def report(self):
        if not self.rows:
            return
        print("\nper launch: mode, worst err/bound, must-inf / must-finite / undecided / ref-nonfinite per format")
        fam = {}
        for name, mode, worst, counts, dt in self.rows:
            cs = "  ".join(f"{f} {worst[f]:.4f} " + "/".join(str(counts[f][k]) for k in
                                                              ("must_inf", "must_finite", "undecided", "ref_nonfinite"))
                           for f in worst)
            print(f"  {mode:9s} {cs}  {dt:5.1f} s  {name}")
            key = (name.split("-")[0], mode)
            w, c = fam.get(key, (0.0, [0, 0, 0, 0]))
            for f in worst:
                c = [x + counts[f][k] for x, k in zip(c, ("must_inf", "must_finite", "undecided", "ref_nonfinite"))]
            fam[key] = (max(w, max(worst.values())), c)
        print("per family and mode: worst err/bound, summed counts")
        for (f, mode), (w, c) in sorted(fam.items()):
            print(f"  {f:34s} {mode:9s} {w:.4f}  " + " / ".join(str(x) for x in c))
        secs = [r[4] for r in self.rows]
        print(f"{len(secs)} launches, {sum(secs):.1f} s, slowest {max(secs):.2f} s")
