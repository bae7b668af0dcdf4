"""The per-window loss record of a training run, kept on the device (libir2rgb_hip.so: loss_log.hip).

The reference appends ``loss_G.item()`` and ``loss_D.item()`` to two lists every window and reads every term every
``print_freq`` windows (train_vid2vid.py:99-100, :119-127): a host round trip per window.  ``LossLog.push`` hands the
addresses of the scalars ``train_window`` returned to one small kernel instead; ``read`` -- the only call that
synchronises -- fetches the last values and the fp64 means since the previous ``read``; ``history`` returns a term's
column of the ring in window order, which is what the reference's two lists are plotted from.
"""
import ctypes

import numpy as np
import torch

from . import _lib

MAX_NAMES = 32                       # IR2RGB_LOSS_LOG_SLOTS
ABSENT = float(np.float32(-3.402823466e+38))      # IR2RGB_LOSS_LOG_ABSENT: a term that was not in a window


class _HostPointers:
    """A host array of addresses the fastcall bindings take as a pointer (``_addr``)."""

    def __init__(self, n):
        self.array = (ctypes.c_void_p * n)()
        self._addr = ctypes.addressof(self.array)
        self._as_parameter_ = ctypes.c_void_p(self._addr)      # (the plain ctypes binding)


def check_arguments(n_sources, capacity):
    """What ``ir2rgb_loss_log_push`` refuses, refused before a device is touched."""
    if isinstance(capacity, bool) or not isinstance(capacity, int) or capacity <= 0:
        raise ValueError(f"LossLog: capacity is a positive count of windows, got {capacity!r}")
    if not 0 < n_sources <= MAX_NAMES:
        raise ValueError(f"LossLog: between 1 and {MAX_NAMES} loss terms, got {n_sources}")


class LossLog:
    """``names``: the terms to record (at most 32; a window that lacks one -- the temporal scales are inactive in the first
    windows of a sequence -- leaves ``ABSENT`` in its ring row and the term's sum alone).  ``capacity``: windows the ring
    holds."""

    def __init__(self, device, names, capacity=4096):
        names = list(names)
        check_arguments(len(names), capacity)
        if len(set(names)) != len(names):
            raise ValueError("LossLog: a name appears twice")
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError("LossLog: GPU only (no CPU fallback)")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device, self.names, self.capacity = device, names, capacity
        self.slot = {n: i for i, n in enumerate(names)}
        self.ring = torch.full((capacity, MAX_NAMES), ABSENT, dtype=torch.float32, device=device)
        assert ctypes.sizeof(_lib.LossLogState) % 8 == 0
        self.state = torch.zeros(ctypes.sizeof(_lib.LossLogState) // 8, dtype=torch.int64, device=device)
        self._srcs, self._opts = _HostPointers(MAX_NAMES), _HostPointers(8)

    def push(self, out, scaler=None, optimizers=None):
        """One window: ``out`` maps names to zero-dimensional fp32 tensors on the device (what ``train_window`` returns;
        names this log does not record are ignored).  With the trainer's ``LossScaler`` a window whose optimizer steps
        were skipped is counted as skipped and kept out of the sums.  ``optimizers``: the optimizers stepped this window
        whose steps were decided on the device (loss-scaled or guarded: ``Vid2VidTrainer.decided_optimizers``) --
        given, they are asked instead of the scaler, so that a guarded window counts without one.  Does not synchronise."""
        present = 0
        srcs = self._srcs.array
        for name, i in self.slot.items():
            t = out.get(name)
            if t is None:
                continue
            if t.dim() != 0 or t.dtype != torch.float32 or t.device != self.device:
                raise ValueError(f"LossLog.push: {name} is not a zero-dimensional fp32 tensor on {self.device}")
            srcs[i] = t.data_ptr()
            present |= 1 << i
        n_opts = 0
        if optimizers is not None or scaler is not None:
            opts = list(optimizers) if optimizers is not None else scaler.last_optimizers()
            if len(opts) > 8:
                raise ValueError("LossLog.push: at most 8 optimizers")
            for o in opts:
                self._opts.array[n_opts] = o.scaled_state().data_ptr()
                n_opts += 1
        _lib.launch("ir2rgb_loss_log_push", self.ring, self._srcs, present, len(self.names), self.ring, self.capacity,
                    self.state, self._opts if n_opts else None, n_opts)

    def _fetch_state(self):
        return _lib.struct_from_device(_lib.LossLogState, self.state)

    def read(self):
        """-> {"count": windows pushed so far, "skipped": windows skipped since the previous read, "last": {name: value},
        "mean": {name: fp64 mean since the previous read}} -- a term absent from the last window / from every window
        since the previous read is left out of ``last`` / ``mean``.  Synchronises, and zeroes the sums on the device."""
        st = self._fetch_state()
        out = {"count": int(st.count), "skipped": int(st.skipped), "last": {}, "mean": {}}
        if st.count:
            row = self.ring[(st.count - 1) % self.capacity].cpu().numpy()
            for name, i in self.slot.items():
                if row[i] != np.float32(ABSENT):
                    out["last"][name] = float(row[i])
        for name, i in self.slot.items():
            if st.n[i]:
                out["mean"][name] = st.sum[i] / st.n[i]
        self.state[:2 * MAX_NAMES + 1].zero_()         # sums, per-slot counts, skipped; the window count stays
        return out

    def history(self, name):
        """The term's values of the last ``min(count, capacity)`` windows, oldest first, as a 1-D fp32 CPU tensor
        (``ABSENT`` where a window did not have the term).  Synchronises."""
        count = int(self.state[-1].item())
        col = self.ring[:, self.slot[name]].cpu()
        if count <= self.capacity:
            return col[:count].clone()
        k = count % self.capacity
        return torch.cat([col[k:], col[:k]])
