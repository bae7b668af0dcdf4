"""Geometry manifest of the benchmarked training window (test-only).

Every convolution and BatchNorm launch of ``bench.py``'s configuration -- ``Vid2VidTrainer(n_scales_spatial=2)`` on a
512 x 1024 synthetic sequence, bf16, windows 0..13 -- is recorded by two test-side hooks and nothing in the product:

* ``conv._prof_begin`` is wrapped: the general (``conv.py``) and the planned (``stageplan.py``) paths both call it for
  every forward, channel-slice and weight-gradient launch while ``conv.PROFILE`` is a dict;
* ``_lib.lib`` is replaced by a proxy whose convolution and BatchNorm entry points note what they were handed (which
  pointers were NULL, every integer) before calling through.

FlowNet2 runs inline and uncaptured (``IR2RGB_FLOW_STREAM=0``, ``IR2RGB_FLOWNET_GRAPH=0``) so its launches are seen too.
``tests/window_geometries.json`` is the committed result; ``python -m oracle.window --write`` regenerates it on a GPU.
"""
import contextlib
import json
import os

CONV_ENTRIES = {"ir2rgb_conv2d_fwd": "fwd", "ir2rgb_conv2d_fwd_ws": "fwd_ws", "ir2rgb_conv2d_wgrad": "wgrad",
                "ir2rgb_conv2d_wgrad_acc": "wgrad_acc"}
BN_ENTRIES = ("ir2rgb_bn_finalize", "ir2rgb_bn_finalize_ex", "ir2rgb_bn_finalize_apply", "ir2rgb_bn_apply",
              "ir2rgb_bn_bwd")
DESC_FIELDS = ("N", "Hin", "Win", "Cin", "Hout", "Wout", "Cout", "kh", "kw", "stride_h", "stride_w", "pad_h", "pad_w",
               "pad_mode", "transposed", "dtype", "act", "out_f32", "ldx", "ci_off", "ldy", "co_off", "stats_per_sample")
H, W = 512, 1024
N_WINDOWS = 14
ENV = {"IR2RGB_FLOW_STREAM": "0", "IR2RGB_FLOWNET_GRAPH": "0"}
MANIFEST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "window_geometries.json")


def desc_dict(desc):
    return {f: int(getattr(desc, f)) for f in DESC_FIELDS}


def prof_key(rec):
    """conv._prof_key of a conv record (+ "wgrad" for weight-gradient launches), as a tuple."""
    d = rec["desc"]
    key = (d["Cin"], d["Hin"], d["Win"], d["Cout"], d["kh"], d["kw"], d["stride_h"], d["pad_mode"], d["transposed"])
    return key + ("wgrad",) if rec["entry"].startswith("wgrad") else key


def canon(rec):
    return json.dumps(rec, sort_keys=True)


def _given(p):
    """A pointer argument that is not NULL (None / 0)."""
    return not (p is None or (isinstance(p, int) and p == 0))


class _Proxy:
    def __init__(self, real, sink):
        self._real, self._sink = real, sink

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name in CONV_ENTRIES:
            return self._conv(name, fn)
        if name in BN_ENTRIES:
            return self._bn(name, fn)
        return fn

    def _conv(self, name, fn):
        from ir2rgb_amd import conv as C
        sink = self._sink

        def call(desc, *a):
            entry = CONV_ENTRIES[name]
            rec = {"kind": "conv", "entry": entry, "desc": desc_dict(desc)}
            if entry.startswith("wgrad"):
                rec["kernel"] = "conv_wgrad"
            else:
                # (x, wpacked, bias, y, stats[, ws, ws_bytes], stream)
                rec["kernel"] = C.kernel_name(desc)
                rec["bias"], rec["stats"] = _given(a[2]), _given(a[4])
                rec["workspace"] = entry == "fwd_ws" and _given(a[5])
            sink.append(rec)
            return fn(desc, *a)
        return call

    def _bn(self, name, fn):
        from ir2rgb_amd import _lib
        sink = self._sink
        argtypes = _lib.PROTOTYPES[name][1]

        def call(*a):
            args = []
            for t, v in zip(argtypes, a):
                if t is _lib.c_void_p:
                    args.append(_given(v))
                elif t is _lib.c_float:
                    args.append(round(float(v), 6))
                else:
                    args.append(int(v))
            sink.append({"kind": "bn", "entry": name, "args": args[:-1]})   # (the stream is no geometry)
            return fn(*a)
        return call


@contextlib.contextmanager
def recording(sink, keys):
    """Hooks on while inside: conv / BN records go to ``sink`` (list), _prof_begin keys to ``keys`` (set)."""
    from ir2rgb_amd import _lib
    from ir2rgb_amd import conv as C
    real_lib, real_begin, real_prof = _lib.lib, C._prof_begin, C.PROFILE
    proxy = _Proxy(real_lib(), sink)

    def begin(desc, tag=None):
        keys.add(C._prof_key(desc) + ((tag,) if tag else ()))
        return real_begin(desc, tag)
    _lib.lib, C._prof_begin, C.PROFILE = (lambda: proxy), begin, {}
    try:
        yield
    finally:
        _lib.lib, C._prof_begin, C.PROFILE = real_lib, real_begin, real_prof


def run_window(dev, n_windows=N_WINDOWS, dtype=None):
    """Records windows 0..n_windows-1 of the bench configuration.  The caller sets ENV before anything builds FlowNet2.
    Returns (distinct records sorted, _prof_begin key set)."""
    import torch
    from ir2rgb_amd import vid2vid as V
    sink, keys = [], set()
    with recording(sink, keys):
        tr = V.Vid2VidTrainer(dev, seed=0, n_scales_spatial=2, compute_dtype=dtype or torch.bfloat16,
                              resident_inputs=True)
        A, B = V.synthetic_sequence(n_windows + 2, H, W, 1234, dev)
        torch.cuda.synchronize()
        for i in range(n_windows):
            tr.train_window(A[:, i:i + 3], B[:, i:i + 3])
        torch.cuda.synchronize()
    seen = {canon(r): r for r in sink}
    return [seen[k] for k in sorted(seen)], keys


def load():
    with open(MANIFEST) as f:
        return json.load(f)


def conv_entries(manifest=None):
    return [r for r in (manifest or load())["launches"] if r["kind"] == "conv"]


def bn_entries(manifest=None):
    return [r for r in (manifest or load())["launches"] if r["kind"] == "bn"]


def launch_id(rec):
    """Short readable test id of a record."""
    if rec["kind"] == "bn":
        return rec["entry"].replace("ir2rgb_", "") + "-" + "x".join(str(v) for v in rec["args"] if not isinstance(v, bool))
    d = rec["desc"]
    s = (f"{rec['entry']}-{d['N']}x{d['Cin']}x{d['Hin']}x{d['Win']}-{d['Cout']}-k{d['kh']}x{d['kw']}s{d['stride_h']}"
         f"x{d['stride_w']}p{d['pad_h']}x{d['pad_w']}m{d['pad_mode']}t{d['transposed']}a{d['act']}")
    if d["out_f32"]:
        s += "-f32"
    if d["ldx"] or d["ldy"]:
        s += f"-v{d['ldx']}.{d['ci_off']}.{d['ldy']}.{d['co_off']}"
    if d["stats_per_sample"]:
        s += "-sps"
    for flag in ("bias", "stats", "workspace"):
        if rec.get(flag):
            s += "-" + flag[0]
    return s


def main():
    import argparse
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", action="store_true", help="rewrite tests/window_geometries.json")
    ap.add_argument("--out", default=None, help="write the manifest here instead")
    args = ap.parse_args()
    os.environ.update(ENV)
    dev = torch.device("cuda:0")
    recs, keys = run_window(dev)
    man = {"config": {"H": H, "W": W, "n_scales_spatial": 2, "dtype": "bf16", "windows": N_WINDOWS, "env": ENV},
           "launches": recs}
    print(f"{len(recs)} distinct launches, {len(keys)} _prof_begin keys")
    missing = {prof_key(r) for r in recs if r["kind"] == "conv"} ^ keys
    print("prof-key mismatch between hooks:", sorted(missing, key=str))
    path = args.out or (MANIFEST if args.write else None)
    if path:
        with open(path, "w") as f:
            f.write("{\n" + f' "config": {json.dumps(man["config"], sort_keys=True)},\n "launches": [\n')
            f.write(",\n".join("  " + json.dumps(r, sort_keys=True) for r in recs))
            f.write("\n ]\n}\n")
        print("wrote", path)


if __name__ == "__main__":
    main()
