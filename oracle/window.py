"""Geometry manifest of the benchmarked training window (test-only).

Every convolution and BatchNorm launch of ``bench.py``'s configuration -- ``Vid2VidTrainer(n_scales_spatial=2)`` on a
512 x 1024 synthetic sequence, bf16, windows 0..13 -- is recorded by two test-side hooks and nothing in the product:

* ``conv._prof_begin`` is wrapped: the general (``conv.py``) and the planned (``stageplan.py``) paths both call it for
  every forward, channel-slice and weight-gradient launch while ``conv.PROFILE`` is a dict;
* ``_lib.lib`` is replaced by a proxy whose convolution and BatchNorm entry points note what they were handed (which
  pointers were NULL, every integer) before calling through.

FlowNet2 runs inline and uncaptured (``IR2RGB_FLOW_STREAM=0``, ``IR2RGB_FLOWNET_GRAPH=0``) so its launches are seen too.
Every other ``ir2rgb_*`` entry point that launches work is recorded by the same proxy as a ``"kind": "op"`` record:
its integers, which pointers were NULL and its floats (rounded to 6 decimals), without the stream.  Two are decoded:
``loss_multi_fwd/bwd`` records each item of its array (kind, n, hw, chw, weight, target, slot, which of b / ga / mask
were given), and ``adam_step`` copies its device table back and records lr, betas, eps, the block count and a sorted
histogram of (n, all four pointers 16-byte aligned) -- not the step count, which changes every window.  The packing
launches (``conv2d_pack_*``) are left unrecorded: test_losses_gpu.py's batched-repack test covers them.
``entry_class`` sorts every entry of ``_lib.PROTOTYPES`` into conv, bn, pack, query or op.

``tests/window_geometries.json`` is the committed result; ``python -m oracle.window --write`` regenerates it on a GPU.
Its records are replayed against fp64 by oracle/replay_kernels.py (conv, bn) and oracle/replay_ops.py (op).
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
PACK_ENTRIES = ("ir2rgb_conv2d_pack_weight", "ir2rgb_conv2d_pack_weight_adjoint", "ir2rgb_conv2d_pack_batch_build",
                "ir2rgb_conv2d_pack_batch_run")
QUERY_SUFFIXES = ("_elems", "_bytes", "_rows", "_blocks")
QUERY_ENTRIES = ("ir2rgb_conv2d_kernel_name", "ir2rgb_correlation_out_shape", "ir2rgb_version", "ir2rgb_adam_chunk_elems",
                 "ir2rgb_loss_partial_elems")
ADAM_ROW_BYTES = 40        # { float *p; const float *g; float *m; float *v; long n; }
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


def entry_class(name):
    """"conv", "bn", "pack" (unrecorded), "query" (no launch) or "op" for an entry of _lib.PROTOTYPES."""
    if name in CONV_ENTRIES:
        return "conv"
    if name in BN_ENTRIES:
        return "bn"
    if name in PACK_ENTRIES:
        return "pack"
    if name in QUERY_ENTRIES or name.endswith(QUERY_SUFFIXES):
        return "query"
    return "op"


def _ptr(p):
    return p.data_ptr() if hasattr(p, "data_ptr") else int(p or 0)


def _d2h(ptr, nbytes):
    """Bytes at a device address (test-only: synchronizes the device first).  hipMemcpy is looked up through the
    library's own handle, i.e. in the HIP runtime it is linked against."""
    import ctypes
    import torch
    from ir2rgb_amd import _lib
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("oracle.window: a decoded launch inside a graph capture")
    torch.cuda.synchronize()
    buf = ctypes.create_string_buffer(nbytes)
    memcpy = _lib.lib().ctypes_handle.hipMemcpy
    memcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    memcpy.restype = ctypes.c_int
    rc = memcpy(buf, ctypes.c_void_p(ptr), nbytes, 2)      # hipMemcpyDeviceToHost
    if rc != 0:
        raise RuntimeError(f"oracle.window: hipMemcpy failed ({rc})")
    return buf.raw


def _loss_items(items, count):
    out = []
    for i in range(count):
        it = items[i]
        out.append({"kind": int(it.kind), "n": int(it.n), "hw": int(it.hw), "chw": int(it.chw),
                    "weight": round(float(it.weight), 6), "target": round(float(it.target), 6), "slot": int(it.slot),
                    "b": _given(it.b), "ga": _given(it.ga), "mask": _given(it.mask)})
    return out


def _adam_record(a):
    """(table, blocks, nblocks, lr, beta1, beta2, eps, step, stream) -> record fields."""
    import numpy as np
    nblocks = int(a[2])
    blocks = np.frombuffer(_d2h(_ptr(a[1]), 8 * nblocks), dtype=np.int32).reshape(nblocks, 2)
    ntensors = int(blocks[:, 0].max()) + 1
    rows = np.frombuffer(_d2h(_ptr(a[0]), ADAM_ROW_BYTES * ntensors), dtype=np.int64).reshape(ntensors, 5)
    hist = {}
    for p, g, m, v, n in rows.tolist():
        key = (int(n), all(x % 16 == 0 for x in (p, g, m, v)))
        hist[key] = hist.get(key, 0) + 1
    return {"lr": round(float(a[3]), 6), "beta1": round(float(a[4]), 6), "beta2": round(float(a[5]), 6),
            "eps": round(float(a[6]), 9), "nblocks": nblocks,
            "tensors": [[n, al, c] for (n, al), c in sorted(hist.items())]}


class _Proxy:
    def __init__(self, real, sink):
        self._real, self._sink = real, sink

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name in CONV_ENTRIES:
            return self._conv(name, fn)
        if name in BN_ENTRIES:
            return self._bn(name, fn)
        if name.startswith("ir2rgb_") and entry_class(name) == "op":
            return self._op(name, fn)
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

    def _op(self, name, fn):
        import ctypes
        from ir2rgb_amd import _lib
        sink = self._sink
        argtypes = _lib.PROTOTYPES[name][1]

        def call(*a):
            rec = {"kind": "op", "entry": name}
            if name in ("ir2rgb_loss_multi_fwd", "ir2rgb_loss_multi_bwd"):
                # (items, count, dtype, partial, out | gout, stream)
                rec.update(count=int(a[1]), dtype=int(a[2]), items=_loss_items(a[0], int(a[1])))
            elif name == "ir2rgb_adam_step":
                rec.update(_adam_record(a))
            else:
                args = []
                for t, v in zip(argtypes, a):
                    if t is _lib.c_void_p:
                        args.append(_given(v))
                    elif t is _lib.c_float:
                        args.append(round(float(v), 6))
                    elif t in (_lib.c_int, _lib.c_long, ctypes.c_uint):
                        args.append(int(v))
                    else:
                        raise TypeError(f"oracle.window: {name}: argument type {t} not recorded")
                rec["args"] = args[:-1]     # (the stream is no geometry)
            sink.append(rec)
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


def op_entries(manifest=None):
    return [r for r in (manifest or load())["launches"] if r["kind"] == "op"]


def launch_id(rec):
    """Short readable test id of a record."""
    if rec["kind"] == "op":
        s = rec["entry"].replace("ir2rgb_", "")
        if "items" in rec:     # dtype, item count, kinds, slots, elements, items with a gradient
            its = rec["items"]
            return s + (f"-d{rec['dtype']}-{len(its)}items-k{''.join(sorted({str(i['kind']) for i in its}))}"
                        f"-s{''.join(sorted({str(i['slot']) for i in its}))}-n{sum(i['n'] for i in its)}"
                        f"-g{sum(i['ga'] for i in its)}")
        if "tensors" in rec:
            return s + f"-{len(rec['tensors'])}classes-{rec['nblocks']}blocks"
        return s + "-" + "x".join(str(int(v)) if isinstance(v, bool) else str(v) for v in rec["args"])
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
