"""Adam over a parameter list as ONE launch per step (libir2rgb_hip.so: adam.hip).

Same update as ``torch.optim.Adam(params, lr, betas, eps=1e-8)`` with weight_decay 0 and amsgrad off,
which is what the reference builds (generator.py / discriminator.py ``torch.optim.Adam(params, lr=opt.lr,
betas=(opt.beta1, 0.999))``).  Moments live in two flat fp32 buffers; a device table of
{param, grad, exp_avg, exp_avg_sq, numel} rows is refreshed with the current gradient pointers before
every step (one small asynchronous copy from pinned memory).

``FusedAdam.step(scaler, guard)`` is the checked step (adam.hip), decided on the device.  f16 training scales its losses
(``LossScaler``): the step checks the scaled gradient, steps on ``g * inv_scale`` or skips, and ``LossScaler.update``
(loss_scale.hip) applies ``torch._amp_update_scale_``'s rule.  ``GradGuard`` guards the steps of every compute dtype: the
step is skipped on an inf or NaN and a finite gradient is clipped to a global L2 norm, with or without a scaler.  The
decision, the step count and the scale never visit the host.

``ParamEMA`` (libir2rgb_hip.so: ema.hip) keeps an exponential moving average of a parameter list in one more launch per
step; after a loss-scaled step it reads that step's skip decision from the optimizer's device state.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from . import streamcheck as SC


def _chunk_blocks(params, device):
    """The (tensor, chunk) pairs of a parameter list, one per workgroup of a table kernel -> int32 [nblocks, 2]."""
    chunk = _lib.lib().ir2rgb_adam_chunk_elems()
    blocks = [(i, c) for i, p in enumerate(params) for c in range((p.numel() + chunk - 1) // chunk)]
    return torch.tensor(blocks, dtype=torch.int32, device=device).reshape(-1, 2)


class FusedAdam:
    def __init__(self, params, lr=2e-4, betas=(0.5, 0.999), eps=1e-8):
        self.params = [p for p in params if p.requires_grad]
        if not self.params:
            raise ValueError("FusedAdam: no trainable parameters")
        dev = self.params[0].device
        if dev.type != "cuda":
            raise ValueError("FusedAdam: GPU parameters only (no CPU fallback)")
        for p in self.params:
            if p.dtype != torch.float32 or not p.is_contiguous() or p.device != dev:
                raise ValueError("FusedAdam: contiguous fp32 parameters on one device")
        # one parameter group, in torch.optim's shape: Model.update_learning_rate (base_model.py:103-108) walks
        # ``optimizer.param_groups`` and assigns ``param_group['lr']``; the step reads lr / betas / eps from here
        self.param_groups = [{"params": self.params, "lr": lr, "betas": tuple(betas), "eps": eps, "weight_decay": 0,
                              "amsgrad": False}]
        self.step_count = 0
        n = sum(p.numel() for p in self.params)
        self.exp_avg = torch.zeros(n, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(n, dtype=torch.float32, device=dev)
        rows = np.zeros((len(self.params), 5), dtype=np.int64)
        off = 0
        for i, p in enumerate(self.params):
            k = p.numel()
            rows[i] = (p.data_ptr(), 0, self.exp_avg.data_ptr() + 4 * off, self.exp_avg_sq.data_ptr() + 4 * off, k)
            off += k
        # two pinned staging copies used alternately: the host may run a step ahead of the GPU, and a
        # staging buffer is rewritten only after the asynchronous copy that last read it has completed
        self._rows_host = [torch.from_numpy(rows.copy()).pin_memory() for _ in range(2)]
        self._rows_np = [t.numpy() for t in self._rows_host]
        self._copied = [None, None]
        self._rows_dev = torch.empty_like(self._rows_host[0], device=dev)
        self._blocks = _chunk_blocks(self.params, dev)
        self._ptrs = [p.data_ptr() for p in self.params]
        self.device = dev
        self._flip = 0
        # checked steps only (scaled_state): ir2rgb_adam_state on the device and the check kernel's partial rows
        self._state = self._partial = None
        self._on_device = False          # the step count lives in _state[0] (checked steps) / in step_count
        # the last step() took a scaler or a guard: its skip decision is in scaled_state() (ParamEMA.update, LossLog.push)
        self.last_step_scaled = False

    @property
    def lr(self):
        return self.param_groups[0]["lr"]

    @lr.setter
    def lr(self, value):
        self.param_groups[0]["lr"] = value

    @property
    def betas(self):
        return self.param_groups[0]["betas"]

    @property
    def eps(self):
        return self.param_groups[0]["eps"]

    def zero_grad(self, set_to_none=True):
        for p in self.params:
            if set_to_none:
                p.grad = None
            elif p.grad is not None:
                p.grad.zero_()

    def state_dict(self):
        """torch.optim.Adam's layout ({'state': {i: {'step', 'exp_avg', 'exp_avg_sq'}}, 'param_groups': [...]}), so a
        checkpoint written here loads into torch.optim.Adam over the same parameter list and vice versa."""
        state = {}
        self._read_step_count()
        if self.step_count:
            for i in range(len(self.params)):
                m, v = self.moments(i)
                state[i] = {"step": torch.tensor(float(self.step_count)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
        g = {k: v for k, v in self.param_groups[0].items() if k != "params"}
        g["params"] = list(range(len(self.params)))
        return {"state": state, "param_groups": [g]}

    def load_state_dict(self, sd):
        g = sd["param_groups"][0]
        if len(g["params"]) != len(self.params):
            raise ValueError("FusedAdam.load_state_dict: parameter count differs")
        self.param_groups[0].update({k: v for k, v in g.items() if k in ("lr", "betas", "eps")})
        self.param_groups[0]["betas"] = tuple(self.param_groups[0]["betas"])
        steps = {int(s["step"]) for s in sd["state"].values()}
        if len(steps) > 1:
            raise ValueError("FusedAdam.load_state_dict: parameters with different step counts (one launch updates all)")
        self.step_count = steps.pop() if steps else 0
        self._on_device = False          # (the next loss-scaled step seeds the device state from step_count)
        with torch.no_grad():
            if not sd["state"]:         # a state saved before the first step: start from zero moments, as torch.optim.Adam does
                self.exp_avg.zero_()
                self.exp_avg_sq.zero_()
            for i, s in sd["state"].items():
                m, v = self.moments(int(i))
                m.copy_(s["exp_avg"])
                v.copy_(s["exp_avg_sq"])

    def moments(self, i):
        """(exp_avg, exp_avg_sq) views of parameter i (for tests / checkpoints)."""
        off = sum(p.numel() for p in self.params[:i])
        k = self.params[i].numel()
        return self.exp_avg[off:off + k].view_as(self.params[i]), self.exp_avg_sq[off:off + k].view_as(self.params[i])

    def scaled_state(self):
        """The optimizer's device state of loss-scaled steps (ir2rgb_adam_state as an int32 tensor: ``[0]`` is the count of
        steps taken, seeded from ``step_count``), created on first use together with the check kernel's partial rows."""
        if self._state is None:          # allocated once: LossScaler.update keeps its address
            nbytes = _lib.query("ir2rgb_loss_scale_state_bytes", 0)
            assert ctypes.sizeof(_lib.AdamState) == nbytes
            self._state = torch.zeros(nbytes // 4, dtype=torch.int32, device=self.device)
            nbytes = _lib.query("ir2rgb_grad_check_partial_bytes", self._blocks.shape[0])
            self._partial = torch.zeros(nbytes // 8, dtype=torch.float64, device=self.device)
        if not self._on_device:
            _lib.struct_to_device(_lib.AdamState(step=self.step_count), self._state)
            self._on_device = True
        return self._state

    def _read_step_count(self):
        """``step_count`` from the device state when loss-scaled steps have been counting there (synchronises)."""
        if self._on_device:
            self.step_count = int(self._state[0].item())

    def grad_stats(self):
        """(found_inf, unscaled gradient norm) of the last loss-scaled step (synchronises)."""
        st = _lib.struct_from_device(_lib.AdamState, self.scaled_state())
        return bool(st.found_inf), math.sqrt(st.grad_sumsq) if st.grad_sumsq >= 0 else float("nan")

    def _refresh_table(self):
        """The current gradient pointers into the device table (one asynchronous copy from pinned memory)."""
        k = self._flip
        self._flip ^= 1
        if self._copied[k] is not None:
            self._copied[k].synchronize()
        rows = self._rows_np[k]
        for i, p in enumerate(self.params):
            g = p.grad
            if g is None:
                raise RuntimeError("FusedAdam.step: a parameter has no gradient (FlatGrads assigns zeros to unused ones)")
            if g.dtype != torch.float32 or not g.is_contiguous():
                g = p.grad = g.float().contiguous()
            if p.data_ptr() != self._ptrs[i]:
                raise RuntimeError("FusedAdam.step: parameter storage moved since construction")
            rows[i, 1] = g.data_ptr()
        self._rows_dev.copy_(self._rows_host[k], non_blocking=True)
        if self._copied[k] is None:
            self._copied[k] = torch.cuda.Event()
        self._copied[k].record()

    @torch.no_grad()
    def step(self, scaler=None, guard=None):
        """One Adam step.  Plain (neither argument): the host evaluates the coefficients, one launch.  Checked: with a
        ``LossScaler`` the gradients are those of the scaled loss; with a ``GradGuard`` a finite gradient is clipped to the
        guard's global norm.  Either way the gradient is checked on the device (ir2rgb_grad_check) and the step is taken on
        ``g * factor`` or -- an inf or NaN anywhere -- not at all (ir2rgb_adam_step_checked); the host learns neither."""
        if guard is not None and guard.optimizer is not self:
            raise ValueError("FusedAdam.step: the guard was built for another optimizer")
        self._refresh_table()
        nblocks = self._blocks.shape[0]
        self.last_step_scaled = scaler is not None or guard is not None
        if self.last_step_scaled:
            state = self.scaled_state()
            _lib.launch("ir2rgb_grad_check", self.exp_avg, self._rows_dev, self._blocks, nblocks, self._partial, state,
                        None if guard is None else guard.state, None if scaler is None else scaler.state,
                        math.inf if guard is None else guard.max_norm, self.lr, self.betas[0], self.betas[1], self.eps)
            _lib.launch("ir2rgb_adam_step_checked", self.exp_avg, self._rows_dev, self._blocks, nblocks, state)
        else:
            if self._on_device:              # checked steps came before: their count moves back to the host
                self._read_step_count()
                self._on_device = False
            self.step_count += 1
            _lib.launch("ir2rgb_adam_step", self.exp_avg, self._rows_dev.data_ptr(), self._blocks.data_ptr(),
                        nblocks, self.lr, self.betas[0], self.betas[1], self.eps, self.step_count)
        # the kernel wrote the parameters behind autograd's back: bump their version counters so that
        # caches keyed on them (the packed MFMA weights of ir2rgb_amd.layers) are refreshed
        torch.autograd.graph.increment_version(self.params)
        if SC.ENABLED:
            for p in self.params:
                SC.produced(p, "fp32 parameter (Adam step)")


def _fp32_exact(x):
    return float(np.float32(x)) == float(x)


class LossScaler:
    """Loss scale of f16 training, owned by the device (ir2rgb_loss_scale_state: scale, inv_scale, growth tracker, count of
    skipped windows).  ``scale_tensor`` multiplies every loss before its backward pass; each ``FusedAdam.step(scaler)``
    unscales, checks and steps or skips; ``update(optimizers)`` then moves the scale as ``torch.amp.GradScaler`` would:
    times ``backoff_factor`` after a window in which any optimizer saw an inf or NaN, times ``growth_factor`` after
    ``growth_interval`` windows without one.  ``growth_interval=0`` is a static scale (windows that overflow are still
    skipped).  None of this synchronises; ``state_dict`` / ``load_state_dict`` / ``stats`` do.  The factors must be
    exact in fp32 (the kernel receives floats and multiplies in double, as torch does with its doubles)."""

    def __init__(self, device, init_scale=2.0 ** 16, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000):
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError("LossScaler: GPU only (no CPU fallback; loss_scale_update_reference restates the rule)")
        check_scaler_arguments(init_scale, growth_factor, backoff_factor, growth_interval)
        self.device = device
        self.growth_factor, self.backoff_factor, self.growth_interval = float(growth_factor), float(backoff_factor), int(growth_interval)
        assert ctypes.sizeof(_lib.LossScaleState) == _lib.query("ir2rgb_loss_scale_state_bytes", 1)
        self.state = torch.zeros(ctypes.sizeof(_lib.LossScaleState) // 4, dtype=torch.float32, device=device)
        self.scale_tensor = self.state[0]        # 0-dim fp32 view: a device operand of the loss products
        self._write(init_scale, 0, 0)
        self._tables = {}
        self._last = []

    def _write(self, scale, tracker, skipped):
        scale = float(np.float32(scale))
        st = _lib.LossScaleState(scale=scale, inv_scale=float(np.float32(1.0 / scale)), growth_tracker=tracker, skipped=skipped)
        _lib.struct_to_device(st, self.state)

    def _read(self):
        return _lib.struct_from_device(_lib.LossScaleState, self.state)

    def register(self, optimizers):
        """The device table of the optimizers' state addresses ``update`` hands the kernel; built once per set of
        optimizers (a small blocking copy: call it ahead of the loop for an ``update`` that never synchronises)."""
        key = tuple(id(o) for o in optimizers)
        if key not in self._tables:
            if not 1 <= len(optimizers) <= 8:
                raise ValueError("LossScaler.update: between 1 and 8 optimizers")
            self._tables[key] = torch.tensor([o.scaled_state().data_ptr() for o in optimizers], dtype=torch.int64,
                                             device=self.device)
        return self._tables[key]

    def forget_tables(self):
        """Drops every registered table: for a trainer that replaces an optimizer (the tables are keyed by the optimizers'
        identities, and hold the addresses of their device state)."""
        self._tables = {}
        self._last = []

    def last_optimizers(self):
        """The optimizers of the last ``update``: the ones stepped in the last window."""
        return list(self._last)

    def update(self, optimizers):
        """Once per window, after the ``step(scaler)`` of every optimizer in ``optimizers``."""
        optimizers = list(optimizers)
        table = self.register(optimizers)
        self._last = optimizers
        _lib.launch("ir2rgb_loss_scale_update", self.state, self.state, table, len(optimizers), self.growth_factor,
                    self.backoff_factor, self.growth_interval)

    def stats(self):
        """{scale, skipped, grad_norms}: the current scale, the windows skipped so far and the unscaled gradient norm each
        optimizer of the last ``update`` saw (synchronises)."""
        st = self._read()
        return {"scale": st.scale, "skipped": st.skipped, "grad_norms": [o.grad_stats()[1] for o in self._last]}

    def state_dict(self):
        st = self._read()
        return {"scale": st.scale, "growth_tracker": st.growth_tracker, "skipped": st.skipped,
                "growth_factor": self.growth_factor, "backoff_factor": self.backoff_factor, "growth_interval": self.growth_interval}

    def load_state_dict(self, sd):
        check_scaler_arguments(sd["scale"], sd.get("growth_factor", self.growth_factor), sd.get("backoff_factor", self.backoff_factor),
                               sd.get("growth_interval", self.growth_interval))
        self.growth_factor = float(sd.get("growth_factor", self.growth_factor))
        self.backoff_factor = float(sd.get("backoff_factor", self.backoff_factor))
        self.growth_interval = int(sd.get("growth_interval", self.growth_interval))
        self._write(sd["scale"], int(sd["growth_tracker"]), int(sd.get("skipped", 0)))


def check_scaler_arguments(scale, growth_factor, backoff_factor, growth_interval):
    if isinstance(scale, bool) or not isinstance(scale, (int, float)) or not math.isfinite(scale) or scale <= 0 or \
            not math.isfinite(float(np.float32(scale))) or float(np.float32(scale)) == 0.0:
        raise ValueError(f"loss scale: a positive finite fp32 number, got {scale!r}")
    if not (growth_factor >= 1.0 and _fp32_exact(growth_factor)) or not (0.0 < backoff_factor <= 1.0 and _fp32_exact(backoff_factor)):
        raise ValueError("loss scale: growth_factor >= 1 and backoff_factor in (0, 1], both exact in fp32")
    if isinstance(growth_interval, bool) or not isinstance(growth_interval, int) or growth_interval < 0:
        raise ValueError("loss scale: growth_interval is a count of windows (0: static scale)")


def check_loss_scale_option(value, fused_adam):
    """Validates the trainer's ``loss_scale`` option -- None, a number (static scale), "dynamic" or a LossScaler -- without
    touching a device.  -> "none" | "static" | "dynamic" | "instance"."""
    if value is None:
        return "none"
    if isinstance(value, LossScaler):
        kind = "instance"
    elif isinstance(value, str):
        if value != "dynamic":
            raise ValueError(f"loss_scale: None, a number, \"dynamic\" or a LossScaler, got {value!r}")
        kind = "dynamic"
    elif isinstance(value, (int, float)) and not isinstance(value, bool):
        check_scaler_arguments(value, 2.0, 0.5, 0)
        kind = "static"
    else:
        raise ValueError(f"loss_scale: None, a number, \"dynamic\" or a LossScaler, got {value!r}")
    if not fused_adam:
        raise ValueError("loss_scale needs fused_adam=True: the skip decision is taken on the device by ir2rgb_amd.optim.FusedAdam")
    return kind


def make_loss_scaler(value, device):
    """The LossScaler of a validated ``loss_scale`` option (None for None)."""
    kind = check_loss_scale_option(value, True)
    if kind == "none":
        return None
    if kind == "instance":
        return value
    if kind == "dynamic":
        return LossScaler(device)
    return LossScaler(device, init_scale=float(value), growth_interval=0)


GUARD_FAMILIES = ("G", "D", "D_T")


def check_max_norm(value, what="max_norm"):
    """A clipping threshold: a number above 0, ``float("inf")`` (guard only, never clip) included -> as a float."""
    if isinstance(value, bool) or not isinstance(value, (int, float)) or math.isnan(value) or value <= 0:
        raise ValueError(f"{what}: a number above 0 (float(\"inf\"): never clip), got {value!r}")
    if float(np.float32(value)) == 0.0:
        raise ValueError(f"{what}: {value!r} is 0 as fp32")
    with np.errstate(over="ignore"):
        return float(np.float32(value))       # (the kernel receives a float)


def check_grad_guard_option(value, fused_adam):
    """Validates the trainer's ``max_grad_norm`` option -- None, a threshold for every optimizer, or a dict of thresholds
    per optimizer family ("G", "D", "D_T"; a missing key means inf) -- without touching a device.
    -> None | {"G": x, "D": y, "D_T": z}."""
    if value is None:
        return None
    if isinstance(value, dict):
        unknown = [k for k in value if k not in GUARD_FAMILIES]
        if unknown:
            raise ValueError(f"max_grad_norm: keys are among {GUARD_FAMILIES}, got {unknown!r}")
        out = {k: check_max_norm(value[k], f"max_grad_norm[{k!r}]") if k in value else math.inf for k in GUARD_FAMILIES}
    else:
        out = dict.fromkeys(GUARD_FAMILIES, check_max_norm(value, "max_grad_norm"))
    if not fused_adam:
        raise ValueError("max_grad_norm needs fused_adam=True: the decision is taken on the device by ir2rgb_amd.optim.FusedAdam")
    return out


class GradGuard:
    """The guard of one ``FusedAdam``: ``optimizer.step(scaler, guard)`` skips the step when the gradient holds an inf or a
    NaN and otherwise clips it to the global L2 norm ``max_norm`` (``float("inf")``: never), decided on the device
    (libir2rgb_hip.so: adam.hip; ``grad_guard_reference`` restates the rule).  Owns the optimizer's
    ir2rgb_grad_guard_state; ``norm_tensor`` is the unscaled gradient norm of the last step as a 0-dim fp32 view of it, a
    device operand for ``LossLog``.  Nothing synchronises but ``stats``."""

    def __init__(self, optimizer, max_norm):
        if not isinstance(optimizer, FusedAdam):
            raise ValueError("GradGuard: the optimizer is an ir2rgb_amd.optim.FusedAdam (the decision is taken by its kernels)")
        self.max_norm = check_max_norm(max_norm, "GradGuard: max_norm")
        self.optimizer = optimizer
        nbytes = _lib.query("ir2rgb_grad_guard_state_bytes")
        assert ctypes.sizeof(_lib.GradGuardState) == nbytes
        self.state = torch.zeros(nbytes // 4, dtype=torch.int32, device=optimizer.device)
        self.norm_tensor = self.state.view(torch.float32)[0]

    def stats(self):
        """{steps, clipped, skipped, grad_norm, clip_coef}: steps taken, steps clipped, steps skipped, and the norm and
        coefficient of the last one checked (synchronises)."""
        st = _lib.struct_from_device(_lib.GradGuardState, self.state)
        return {"steps": st.steps, "clipped": st.clipped, "skipped": st.skipped, "grad_norm": st.grad_norm, "clip_coef": st.clip_coef}


EMA_WARMUP_END = 1 << 20         # csrc/ema.hip: from this update on the decay is beta itself


def check_ema_option(value):
    """Validates the trainer's ``ema_decay`` option -- None (no average) or a number in [0, 1) -- without touching a
    device.  -> the decay as the fp32 number the kernel receives, or None."""
    if value is None:
        return None
    if isinstance(value, bool) or not isinstance(value, (int, float)) or not 0.0 <= float(np.float32(value)) < 1.0:
        raise ValueError(f"ema_decay: None or a number in [0, 1) (as fp32), got {value!r}")
    return float(np.float32(value))


class ParamEMA:
    """Exponential moving average of a parameter list as ONE launch per update (libir2rgb_hip.so: ema.hip):
    ``e <- e + alpha * (p - e)`` with ``alpha = 1 - beta_n`` and ``beta_n = min(beta, (1 + n) / (10 + n))`` for the n-th
    update while ``warmup`` is on.  The averages live in one flat fp32 shadow buffer (each tensor at an offset that is a
    multiple of 4 elements: 16-byte loads for every row), seeded as a bit copy of the parameters.  The count of updates
    and the coefficient live on the device; ``update(optimizer)`` after a loss-scaled ``FusedAdam.step(scaler)`` leaves
    the average alone when that step was skipped -- decided on the device from the optimizer's state.  ``update`` never
    synchronises; ``stats`` / ``state_dict`` / ``load_state_dict`` do."""

    def __init__(self, params, beta, warmup=True):
        self.params = list(params)
        if not self.params:
            raise ValueError("ParamEMA: no parameters")
        self.beta = check_ema_option(beta)
        if self.beta is None:
            raise ValueError("ParamEMA: beta is a number in [0, 1)")
        self.warmup = bool(warmup)
        dev = self.params[0].device
        if dev.type != "cuda":
            raise ValueError("ParamEMA: GPU parameters only (no CPU fallback; ema_reference restates the arithmetic)")
        for p in self.params:
            if p.dtype != torch.float32 or not p.is_contiguous() or p.device != dev:
                raise ValueError("ParamEMA: contiguous fp32 parameters on one device")
        self.device = dev
        self._offsets, off = [], 0
        for p in self.params:
            self._offsets.append(off)
            off += (p.numel() + 3) // 4 * 4
        self.buf = torch.zeros(max(off, 4), dtype=torch.float32, device=dev)
        rows = np.zeros((len(self.params), 3), dtype=np.int64)
        for i, (p, o) in enumerate(zip(self.params, self._offsets)):
            rows[i] = (p.data_ptr(), self.buf.data_ptr() + 4 * o, p.numel())
        self._rows_dev = torch.from_numpy(rows).to(dev)
        self._blocks = _chunk_blocks(self.params, dev)
        self._ptrs = [p.data_ptr() for p in self.params]
        self._views = [self.buf[o:o + p.numel()].view_as(p) for p, o in zip(self.params, self._offsets)]
        nbytes = _lib.query("ir2rgb_ema_state_bytes")
        assert ctypes.sizeof(_lib.EmaState) == nbytes
        self.state = torch.zeros(nbytes // 4, dtype=torch.int32, device=dev)
        self.reseed()

    def shadow(self, i):
        """The average of parameter i: a view of the shadow buffer in the parameter's shape."""
        return self._views[i]

    def _write(self, updates, skipped, alpha=0.0):
        st = _lib.EmaState(updates=int(updates), skipped=int(skipped), alpha=float(alpha))
        _lib.struct_to_device(st, self.state)

    def _read(self):
        return _lib.struct_from_device(_lib.EmaState, self.state)

    def _touched(self):
        # the shadow changed behind autograd's back: caches keyed on the version counter (the packed MFMA weights of
        # modules whose parameters alias the shadow, Vid2VidTrainer.ema_generators) are refreshed on their next use
        torch.autograd.graph.increment_version(self._views)
        if SC.ENABLED:
            for v in self._views:
                SC.produced(v, "fp32 parameter average (EMA)")

    @torch.no_grad()
    def reseed(self):
        """The average becomes a bit copy of the current parameters and ``updates`` 0 (``skipped`` is kept)."""
        skipped = self._read().skipped
        torch._foreach_copy_(self._views, [p.detach() for p in self.params])
        self._write(0, skipped)
        self._touched()

    @torch.no_grad()
    def update(self, optimizer=None):
        """One update, on the current stream.  ``optimizer``: the ``FusedAdam`` that has just stepped these parameters; if
        that step was loss-scaled, its device state tells the kernel whether the step was taken (a skipped step skips the
        average and counts in ``skipped``).  Anything else: the average is always taken."""
        for p, ptr in zip(self.params, self._ptrs):
            if p.data_ptr() != ptr:
                raise RuntimeError("ParamEMA.update: parameter storage moved since construction")
        opt_state = optimizer.scaled_state() if getattr(optimizer, "last_step_scaled", False) else None
        if SC.ENABLED:
            for p in self.params:
                SC.consumed(p, "fp32 parameter (Adam step)")
        _lib.launch("ir2rgb_ema_step", self.buf, self._rows_dev, self._blocks, self._blocks.shape[0], self.state, opt_state,
                    self.beta, int(self.warmup))
        self._touched()

    def stats(self):
        """{updates, skipped, alpha}: averages taken, windows skipped, the coefficient of the last one taken (synchronises)."""
        st = self._read()
        return {"updates": st.updates, "skipped": st.skipped, "alpha": st.alpha}

    def state_dict(self):
        """The counts and the settings they were taken under; the averages themselves are saved as networks
        (ir2rgb_amd.checkpoint)."""
        st = self._read()
        return {"updates": st.updates, "skipped": st.skipped, "beta": self.beta, "warmup": self.warmup}

    def load_state_dict(self, sd):
        """Restores the counts (the warm-up continues where it was).  ``beta`` and ``warmup`` stay this instance's."""
        updates, skipped = int(sd["updates"]), int(sd.get("skipped", 0))
        if updates < 0 or skipped < 0:
            raise ValueError("ParamEMA.load_state_dict: negative counts")
        self._write(updates, skipped, self._read().alpha)


# ---------------------------------------------------------------------------------------------------------------------
# plain torch / numpy restatements, usable on a CPU (what the kernels are tested against; never on the training path)
def ema_beta(n, beta, warmup=True):
    """beta_n of the n-th update (n >= 1) as ema_prepare_kernel evaluates it, in numpy float32."""
    f = np.float32
    if warmup and n < EMA_WARMUP_END:
        return min(f(beta), f(1 + n) / f(10 + n))
    return f(beta)


def ema_reference(e, p, n, beta, warmup=True):
    """ema_kernel's arithmetic in numpy float32, operation by operation: the n-th update (n >= 1) of the average ``e``
    towards ``p`` -> the new average.  ``alpha = 1 - beta_n``, ``d = p - e``, ``t = alpha * d``, ``e + t``, each rounded
    to fp32; inf and NaN propagate."""
    f = np.float32
    e, p = np.asarray(e, dtype=f), np.asarray(p, dtype=f)
    with np.errstate(all="ignore"):
        alpha = f(f(1.0) - ema_beta(n, beta, warmup))
        d = (p - e).astype(f)
        t = (alpha * d).astype(f)
        return (e + t).astype(f)



def loss_scale_update_reference(scale, growth_tracker, found_inf, growth_factor, backoff_factor, growth_interval):
    """loss_scale_update_kernel's rule, in place on a 1-element fp32 ``scale`` and int32 ``growth_tracker``;
    ``found_inf``: any non-zero element means an optimizer skipped.  For ``growth_interval > 0`` this is
    ``torch._amp_update_scale_`` (products in double, rounded to fp32; a growth that would reach inf is refused but
    still resets the tracker); ``growth_interval == 0`` leaves both alone.  -> (inv_scale, 1 if the window was skipped)."""
    found = bool(torch.as_tensor(found_inf).ne(0).any())
    if growth_interval > 0:
        if found:
            scale.copy_((scale.double() * backoff_factor).float())
            growth_tracker.zero_()
        else:
            growth_tracker += 1
            if int(growth_tracker) == growth_interval:
                grown = (scale.double() * growth_factor).float()
                if bool(torch.isfinite(grown).all()):
                    scale.copy_(grown)
                growth_tracker.zero_()
    return (1.0 / scale.double()).float(), int(found)


def grad_guard_reference(grads, max_norm, inv_scale=1.0):
    """grad_check_kernel + grad_check_finish_kernel's rule in torch fp64 on the CPU, over the stored gradients of ONE
    optimizer (those of the scaled loss when ``inv_scale`` is a loss scaler's):
    -> (found, sumsq, norm, c, factor).  ``found``: an element with an all-ones exponent (inf or NaN).  ``sumsq``: the
    fp64 sum of squares of the stored gradients; ``norm = sqrt(sumsq) * inv_scale``; ``c = min(1, max_norm / (norm +
    1e-6))`` (``torch.nn.utils.clip_grad_norm_``'s coefficient, in double); ``factor``: what the step multiplies every
    stored element by, ``inv_scale * c`` rounded to fp32.  After ``found`` the step is skipped and ``c`` and ``factor``
    are 0.  ``max_norm`` and ``inv_scale`` are taken as the fp32 numbers the device holds."""
    flat = [torch.as_tensor(g).detach().cpu().reshape(-1) for g in grads]
    found = any(not bool(torch.isfinite(g).all()) for g in flat)
    sumsq = float(sum(float((g.double() * g.double()).sum()) for g in flat))
    if found:
        inv = float(np.float32(inv_scale))
        return True, sumsq, math.sqrt(sumsq) * inv if sumsq >= 0 else float("nan"), 0.0, 0.0
    return (False, sumsq) + grad_guard_rule(sumsq, max_norm, inv_scale)


def grad_guard_rule(sumsq, max_norm, inv_scale=1.0):
    """What grad_check_finish_kernel derives from a finite gradient's sum of squares, the same expressions in double:
    -> (norm, c, factor), ``factor`` rounded to fp32."""
    inv = float(np.float32(inv_scale))
    norm = math.sqrt(sumsq) * inv
    q = float(np.float32(max_norm)) / (norm + 1e-6)
    c = q if q < 1.0 else 1.0
    return norm, c, float(np.float32(inv * c))


def grad_check_reference(grads, inv_scale):
    """grad_check_kernel + grad_check_finish_kernel in plain torch: -> (found_inf as 0. / 1., the fp64 sum of squares of
    the unscaled gradient, the unscaled gradients ``g * inv_scale`` in fp32).  Finiteness is decided per element."""
    inv = torch.as_tensor(inv_scale, dtype=torch.float32)
    found = any(not bool(torch.isfinite(g).all()) for g in grads)
    sumsq = sum((g.double() ** 2).sum() for g in grads) * inv.double() ** 2
    return (torch.tensor(1.0 if found else 0.0), torch.as_tensor(sumsq, dtype=torch.float64),
            [g.float() * inv for g in grads])
