"""The generator average on the device (csrc/ema.hip, ir2rgb_amd.optim.ParamEMA, the trainer's ``ema_decay``, the ``_ema``
checkpoint files, ``VideoTranslator(weights="ema")``).

Kernel level: ir2rgb_ema_step over the tensor sizes of tests/test_loss_scale_gpu.py (every path of the three-way split, the
chunk boundary from both sides, one tensor off 16-byte alignment) against ``optim.ema_reference`` with tolerance 0 --
tests/test_ema_cpu.py holds that reference to fp64 and shows that a bit comparison sees a fused multiply-add, the other
form of the update and a stale coefficient.  Trainer level: training is bit-reproducible and the average only reads the
parameters, so everything is compared bit for bit as well.
"""
import os
import shutil
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_loss_scale_gpu import CANARY, E, SPECS, _Banded, _pool, _state, _toy, _trainer  # noqa: E402

from ir2rgb_amd import _lib  # noqa: E402
from ir2rgb_amd import checkpoint as CK  # noqa: E402
from ir2rgb_amd import optim as OP  # noqa: E402

F = np.float32
BETA = 0.999
TOP = 1 << 20


def _bits(t):
    return (t if isinstance(t, np.ndarray) else t.numpy()).view(np.int32)


def _same(got, want):
    """Bit-equal, a NaN standing for any NaN."""
    got, want = np.asarray(got, dtype=F), np.asarray(want, dtype=F)
    return (_bits(got) == _bits(want)) | (np.isnan(got) & np.isnan(want))


class _EmaTable:
    """The {p, e, n} table over SPECS, each array in a pool of its own with guard floats on both sides."""

    def __init__(self, dev, host):
        assert _lib.lib().ir2rgb_adam_chunk_elems() == E
        rows, blocks, self.pools = [], [], []
        for i, ((n, aligned), arrs) in enumerate(zip(SPECS, host)):
            pl = [_pool(n, aligned, t, dev) for t in arrs]
            ptrs = [p.data_ptr() + 4 * off for p, off in pl]
            assert all(q % 16 == 0 for q in ptrs) == aligned and all(q % 4 == 0 for q in ptrs)
            rows.append(ptrs + [n])
            blocks += [(i, c) for c in range(-(-n // E))]
            self.pools.append(pl)
        self.table = torch.tensor(rows, dtype=torch.int64, device=dev)
        self.blocks = torch.tensor(blocks, dtype=torch.int32, device=dev)
        self.nblocks = len(blocks)

    def read(self):
        """-> per tensor [p, e] on the host; asserts the guards."""
        out = []
        for (n, aligned), pl in zip(SPECS, self.pools):
            got = []
            for pool, off in pl:
                h = pool.cpu()
                assert torch.all(torch.cat([h[:off], h[off + n:]]) == CANARY), f"n={n} aligned={aligned}: a pool guard was overwritten"
                got.append(h[off:off + n].clone())
            out.append(got)
        return out


def _host_arrays(seed):
    g = torch.Generator().manual_seed(seed)
    return [[torch.randn(n, generator=g) * 0.05, torch.randn(n, generator=g) * 0.05] for n, _ in SPECS]


SPECIALS = [float("inf"), float("-inf"), float("nan"), -0.0, 1e-40, -1.4e-45]    # (the last two: f32 subnormals)


def _plant(host):
    """Specials at the first, the last and the chunk-boundary elements of p and of e; the two cycles are offset so that a
    special meets an ordinary value, another special (inf - inf) and itself."""
    k = 0
    for (n, _), (p, e) in zip(SPECS, host):
        for pos in sorted({0, n - 1} | {q for q in (E - 1, E, 2 * E - 1, 2 * E) if q < n}):
            p[pos] = SPECIALS[k % 6]
            if k % 3:
                e[pos] = SPECIALS[(k // 3) % 6]
            k += 1
        if n > 2 * E:                  # an ordinary p against a special e, mid-chunk
            e[E + 100], e[E + 101], e[E + 102] = float("nan"), float("inf"), 1e-40
    return host


def _step(dev, host, n, beta, warmup, found_inf=None, skipped0=5):
    """ir2rgb_ema_step with ``updates`` preset to n - 1 -> (per tensor [p, e], EmaState, the optimizer state's bytes | None)."""
    tab = _EmaTable(dev, host)
    st = _Banded(dev, _lib.query("ir2rgb_ema_state_bytes"), _lib.EmaState(updates=n - 1, skipped=skipped0, alpha=0.25))
    opt = None
    if found_inf is not None:
        opt = _Banded(dev, _lib.query("ir2rgb_loss_scale_state_bytes", 0), _lib.AdamState(step=3, found_inf=found_inf, grad_sumsq=2.0))
    _lib.launch("ir2rgb_ema_step", tab.table, tab.table, tab.blocks, tab.nblocks, st.ptr, opt.ptr if opt else None, beta, int(warmup))
    torch.cuda.synchronize()
    return tab.read(), _lib.EmaState.from_buffer_copy(st.bytes()), opt.bytes() if opt else None


def _assert_update(host, got, st, n, beta, warmup, what):
    for (size, aligned), (p, e), (p1, e1) in zip(SPECS, host, got):
        assert np.array_equal(_bits(p), _bits(p1)), f"{what} n={size} aligned={aligned}: p was written"
        want = OP.ema_reference(e.numpy(), p.numpy(), n, beta, warmup)
        ok = _same(e1.numpy(), want)
        assert ok.all(), f"{what} n={size} aligned={aligned}: {int((~ok).sum())} elements differ from ema_reference, first at {int(np.argmin(ok))}"
    assert st.updates == n and st.skipped == 5
    assert np.array_equal(_bits(np.array([st.alpha], dtype=F)), _bits(np.array([F(1.0) - OP.ema_beta(n, beta, warmup)], dtype=F)))


@pytest.mark.parametrize("warmup", [True, False])
@pytest.mark.parametrize("n", [1, 2, 9, 8989, 8991, TOP + 3])
def test_step_is_the_reference_bit_for_bit(dev, n, warmup):
    host = _host_arrays(n % 1000)
    got, st, _ = _step(dev, host, n, BETA, warmup)
    _assert_update(host, got, st, n, BETA, warmup, f"update {n} warmup={warmup}")
    again, st2, _ = _step(dev, host, n, BETA, warmup)
    assert bytes(st) == bytes(st2) and all(np.array_equal(_bits(a[1]), _bits(b[1])) for a, b in zip(got, again)), "does not repeat bit for bit"


@pytest.mark.parametrize("n", [9, TOP + 3])
def test_special_values_propagate_as_ieee(dev, n):
    host = _plant(_host_arrays(40 + n % 7))
    got, st, _ = _step(dev, host, n, BETA, True)
    _assert_update(host, got, st, n, BETA, True, f"specials, update {n}")
    e1 = torch.cat([g[1] for g in got])
    assert bool(torch.isnan(e1).any()) and bool(torch.isinf(e1).any())
    again, _, _ = _step(dev, host, n, BETA, True)
    assert all(_same(a[1].numpy(), b[1].numpy()).all() for a, b in zip(got, again))


def test_skip_null_state_empty_launch_and_bad_beta(dev):
    host = _host_arrays(3)
    # a skipped step: e byte for byte as it was, updates as it was, one more skipped window, the optimizer's state only read
    want_opt = bytes(_lib.AdamState(step=3, found_inf=1.0, grad_sumsq=2.0))
    got, st, opt = _step(dev, host, 7, BETA, True, found_inf=1.0)
    assert opt == want_opt
    for (p, e), (p1, e1) in zip(host, got):
        assert np.array_equal(_bits(p), _bits(p1)) and np.array_equal(_bits(e), _bits(e1)), "a skipped update wrote"
    assert (st.updates, st.skipped) == (6, 6) and st.alpha == 0.25
    # a step that was taken, and no optimizer state at all: both update
    got, st, opt = _step(dev, host, 7, BETA, True, found_inf=0.0)
    assert opt == bytes(_lib.AdamState(step=3, found_inf=0.0, grad_sumsq=2.0))
    _assert_update(host, got, st, 7, BETA, True, "found_inf 0")
    got, st, _ = _step(dev, host, 7, BETA, True)
    _assert_update(host, got, st, 7, BETA, True, "NULL optimizer state")
    # nblocks 0: OK and nothing moves; beta 1: refused before any launch; so are NULL tables and a negative count
    tab = _EmaTable(dev, host)
    st = _Banded(dev, _lib.query("ir2rgb_ema_state_bytes"), _lib.EmaState(updates=4, skipped=1, alpha=0.5))
    lib = _lib.lib()
    stream = _lib.current_stream(tab.table)
    assert lib.ir2rgb_ema_step(tab.table, tab.blocks, 0, st.ptr, None, BETA, 1, stream) == 0
    for args in ((tab.table, tab.blocks, tab.nblocks, st.ptr, None, 1.0, 1), (tab.table, tab.blocks, tab.nblocks, st.ptr, None, -0.1, 1),
                 (tab.table, tab.blocks, tab.nblocks, st.ptr, None, float("nan"), 1), (None, tab.blocks, tab.nblocks, st.ptr, None, BETA, 1),
                 (tab.table, None, tab.nblocks, st.ptr, None, BETA, 1), (tab.table, tab.blocks, tab.nblocks, None, None, BETA, 1),
                 (tab.table, tab.blocks, -1, st.ptr, None, BETA, 1)):
        assert lib.ir2rgb_ema_step(*args, stream) == -1, args[2:]
    with pytest.raises(ValueError, match="ema_step"):
        _lib.launch("ir2rgb_ema_step", tab.table, tab.table, tab.blocks, tab.nblocks, st.ptr, None, 1.0, 1)
    torch.cuda.synchronize()
    assert st.bytes() == bytes(_lib.EmaState(updates=4, skipped=1, alpha=0.5))
    for (p, e), (p1, e1) in zip(host, tab.read()):
        assert np.array_equal(_bits(p), _bits(p1)) and np.array_equal(_bits(e), _bits(e1))


# ---------------------------------------------------------------------------------------------------------------------
# ParamEMA
def test_param_ema_layout_update_reseed_and_state(dev):
    params = _toy(dev, 1)                                   # 5, 8193, 100, 3 * 8192 elements
    ema = OP.ParamEMA(params, BETA)
    assert all(ema.shadow(i).data_ptr() % 16 == 0 and ema.shadow(i).shape == p.shape for i, p in enumerate(params))
    assert all(torch.equal(ema.shadow(i), p) for i, p in enumerate(params)) and ema.stats()["updates"] == 0
    e = [p.detach().cpu().numpy().copy() for p in params]
    versions = [ema.shadow(i)._version for i in range(len(params))]
    for n in (1, 2, 3):
        with torch.no_grad():
            for p in params:
                p.add_(torch.randn_like(p) * 0.01)
        ema.update()
        e = [OP.ema_reference(a, p.detach().cpu().numpy(), n, BETA) for a, p in zip(e, params)]
        assert all(np.array_equal(_bits(ema.shadow(i).cpu()), _bits(a)) for i, a in enumerate(e)), n
    assert all(ema.shadow(i)._version > v for i, v in enumerate(versions))
    st = ema.stats()
    assert st["updates"] == 3 and st["skipped"] == 0 and st["alpha"] == float(F(1.0) - OP.ema_beta(3, BETA))
    sd = ema.state_dict()
    assert sd == {"updates": 3, "skipped": 0, "beta": float(F(BETA)), "warmup": True}
    other = OP.ParamEMA(params, BETA)
    other.load_state_dict(sd)
    assert other.state_dict() == sd
    ema.reseed()
    assert all(torch.equal(ema.shadow(i), p) for i, p in enumerate(params)) and ema.stats()["updates"] == 0
    with pytest.raises(ValueError):
        OP.ParamEMA(params, 1.0)


def test_update_never_synchronises(dev):
    params = _toy(dev, 3)
    opt = OP.FusedAdam(params, lr=2e-4, betas=(0.5, 0.999))
    scaler = OP.LossScaler(dev, init_scale=2.0 ** 10)
    ema = OP.ParamEMA(params, BETA)
    x = [torch.randn(p.numel(), device=dev) for p in params]

    def window():
        opt.zero_grad()
        loss = sum((p * t).sum() for p, t in zip(params, x))
        (loss * scaler.scale_tensor).backward()
        opt.step(scaler)
        ema.update(opt)
        scaler.update([opt])

    for _ in range(3):          # allocations, the state blocks, both pinned table copies
        window()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(3):
            window()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert ema.stats()["updates"] == 6 and ema.stats()["skipped"] == 0 and scaler.stats()["skipped"] == 0


# ---------------------------------------------------------------------------------------------------------------------
# the trainer
def _gen_params(tr):
    """Every parameter of every generator, flattened in ParamEMA's order, on the host."""
    return [p.detach().cpu().numpy().ravel().copy() for g in tr.netG for p in g.parameters()]


def _shadows(tr):
    return [tr.ema.shadow(i).cpu().numpy().ravel() for i in range(len(tr.ema.params))]


def _assert_bits(got, want, what):
    assert len(got) == len(want)
    bad = [i for i, (a, b) in enumerate(zip(got, want)) if not np.array_equal(_bits(a), _bits(b))]
    assert not bad, f"{what}: {len(bad)} of {len(got)} tensors differ, first {bad[0]}"


def test_trainer_average_is_the_reference_and_training_is_untouched(dev):
    from ir2rgb_amd import vid2vid as V
    A, Bs = V.synthetic_sequence(5, 64, 128, 3, dev)
    plain, tr = _trainer(dev, torch.bfloat16), _trainer(dev, torch.bfloat16, ema_decay=BETA)
    assert plain.ema is None and tr.ema is not None and len(tr.ema.params) == sum(1 for g in tr.netG for _ in g.parameters())
    with pytest.raises(ValueError):
        plain.ema_generators()
    e = _gen_params(tr)
    _assert_bits(_shadows(tr), e, "the seed")
    for w in range(3):
        la, lb = plain.train_window(A[:, w:w + 3], Bs[:, w:w + 3]), tr.train_window(A[:, w:w + 3], Bs[:, w:w + 3])
        assert la.keys() == lb.keys()
        for k in la:
            assert la[k].item() == lb[k].item(), (w, k, la[k].item(), lb[k].item())
        e = [OP.ema_reference(a, p, w + 1, BETA) for a, p in zip(e, _gen_params(tr))]
        _assert_bits(_shadows(tr), e, f"window {w}")
    for i, (sa, sb) in enumerate(zip(_state(plain), _state(tr))):
        for name, x, y in zip(("parameters", "exp_avg", "exp_avg_sq"), sa, sb):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), f"optimizer {i}: {name} differ with ema_decay"
    assert tr.ema.stats() == {"updates": 3, "skipped": 0, "alpha": float(F(1.0) - OP.ema_beta(3, BETA))}
    gens = tr.ema_generators()
    assert gens is tr.ema_generators() and len(gens) == len(tr.netG)
    for g, live in zip(gens, tr.netG):
        assert list(g.state_dict()) == list(live.state_dict()) and not any(p.requires_grad for p in g.parameters())
        assert all(torch.equal(a, b) for a, b in zip(g.buffers(), live.buffers()))
    assert all(p.data_ptr() == tr.ema.shadow(i).data_ptr() for i, p in enumerate(p for g in gens for p in g.parameters()))


def test_trainer_fixed_coarse_scale_keeps_its_average_until_released(dev):
    from ir2rgb_amd import vid2vid as V
    A, Bs = V.synthetic_sequence(5, 64, 128, 3, dev)
    tr = _trainer(dev, torch.bfloat16, ema_decay=BETA, n_scales_spatial=2, niter_fix_global=1)
    n_coarse = sum(1 for _ in tr.netG[0].parameters())
    e = _gen_params(tr)
    for w in range(3):
        if w == 2:
            tr.update_fixed_params()
        before = _gen_params(tr)
        tr.train_window(A[:, w:w + 3], Bs[:, w:w + 3])
        now = _gen_params(tr)
        e = [OP.ema_reference(a, p, w + 1, BETA) for a, p in zip(e, now)]
        got = _shadows(tr)
        _assert_bits(got, e, f"window {w}")
        moved = [not np.array_equal(a, b) for a, b in zip(before[:n_coarse], now[:n_coarse])]
        if w < 2:               # the coarse generator is fixed: its average is its parameters
            assert not any(moved)
            _assert_bits(got[:n_coarse], now[:n_coarse], f"coarse scale, window {w}")
        else:                   # released: it trains, and its average follows without a new seed
            assert any(moved) and all(m == (not np.array_equal(a, b)) for m, a, b in zip(moved, got[:n_coarse], now[:n_coarse]))
    assert tr.ema.stats()["updates"] == 3


def test_trainer_f16_skipped_window_skips_the_average(dev):
    from ir2rgb_amd import vid2vid as V
    scaler = OP.LossScaler(dev, init_scale=2.0 ** 30)
    tr = _trainer(dev, torch.float16, loss_scale=scaler, ema_decay=BETA)
    A, Bs = V.synthetic_sequence(12, 64, 128, 3, dev)
    g_skipped = any_skipped = updates = 0
    clean = None
    for w in range(30):
        shadow, i = tr.ema.buf.clone(), w % 10
        tr.train_window(A[:, i:i + 3], Bs[:, i:i + 3])
        found = [o.grad_stats()[0] for o in scaler.last_optimizers()]
        any_skipped += any(found)
        st = tr.ema.stats()
        if found[0]:            # the generator's step was skipped: so was its average
            g_skipped += 1
            assert torch.equal(shadow.view(torch.int32), tr.ema.buf.view(torch.int32)), "a skipped window moved the average"
        else:
            updates += 1
            assert not torch.equal(shadow, tr.ema.buf), "a clean window left the average alone"
        assert (st["updates"], st["skipped"]) == (updates, g_skipped)
        if not any(found):
            clean = w
            break
    print("first clean window:", clean, "generator skips", g_skipped, "window skips", any_skipped)
    assert clean is not None and g_skipped >= 1 and updates >= 1
    assert scaler.stats()["skipped"] == any_skipped >= g_skipped
    assert bool(torch.isfinite(tr.ema.buf).all())


# ---------------------------------------------------------------------------------------------------------------------
# checkpoints and inference
def _frames_u8(n, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, (64, 128, 3), generator=g, dtype=torch.uint8) for _ in range(n)]


def test_checkpoint_and_inference_use_the_average(dev, tmp_path):
    from ir2rgb_amd import vid2vid as V
    from ir2rgb_amd.inference import VideoTranslator
    kw = dict(first_layer_gen_filters=64, gen_blocks=2)
    A, Bs = V.synthetic_sequence(5, 64, 128, 3, dev)
    tr = _trainer(dev, torch.bfloat16, ema_decay=BETA, gen_blocks=2)
    for w in range(2):
        tr.train_window(A[:, w:w + 3], Bs[:, w:w + 3])
    full, raw_only = str(tmp_path / "full"), str(tmp_path / "raw_only")
    CK.save_trainer(tr, "latest", full)
    raw = torch.load(CK.network_path(full, "G0", "latest"), weights_only=True)
    avg = torch.load(CK.network_path(full, "G0_ema", "latest"), weights_only=True)
    assert list(raw) == list(avg) and any(not torch.equal(raw[k], avg[k]) for k in raw)
    assert torch.load(os.path.join(full, "latest_ema.pth"), weights_only=True) == tr.ema.state_dict()
    os.makedirs(raw_only)
    for f in os.listdir(full):
        if "ema" not in f:
            shutil.copy(os.path.join(full, f), raw_only)
    # a fresh trainer with other weights takes the average and its count over
    tr2 = _trainer(dev, torch.bfloat16, ema_decay=BETA, gen_blocks=2, seed=5)
    assert not torch.equal(tr2.ema.buf, tr.ema.buf)
    CK.load_trainer(tr2, "latest", full, log=lambda *_: None)
    assert torch.equal(tr2.ema.buf.view(torch.int32), tr.ema.buf.view(torch.int32)) and tr2.ema.stats()["updates"] == 2
    assert all(torch.equal(a, b) for a, b in zip(tr2.netG[0].parameters(), tr.netG[0].parameters()))
    # without the files the average restarts from the parameters just loaded
    lines = []
    tr3 = _trainer(dev, torch.bfloat16, ema_decay=BETA, gen_blocks=2, seed=6)
    tr3.ema.load_state_dict({"updates": 9, "skipped": 0})
    CK.load_trainer(tr3, "latest", raw_only, log=lines.append)
    assert any("G0_ema.pth not exists yet!" in str(l) for l in lines) and any("latest_ema.pth not exists yet!" in str(l) for l in lines)
    assert tr3.ema.stats()["updates"] == 0
    assert all(torch.equal(tr3.ema.shadow(i), p) for i, p in enumerate(p for g in tr3.netG for p in g.parameters()))
    assert all(torch.equal(a, b) for a, b in zip(tr3.netG[0].parameters(), tr.netG[0].parameters()))
    # a trainer without the average ignores the files
    plain = _trainer(dev, torch.bfloat16, gen_blocks=2, seed=7)
    CK.load_trainer(plain, "latest", full, log=lambda *_: None)
    assert plain.ema is None

    frames = _frames_u8(4, 8)
    run = lambda **k: torch.stack(list(VideoTranslator(dev, 64, 128, **kw, **k).translate(frames)))  # noqa: E731
    from_files = run(checkpoint_dir=full, weights="ema")
    from_modules = run(netG=tr.ema_generators(), weights="ema")
    from_raw = run(checkpoint_dir=full, weights="raw")
    assert from_files.shape == (2, 64, 128, 3)
    assert torch.equal(from_files, from_modules), "the saved average and the live one translate differently"
    assert not torch.equal(from_files, from_raw) and torch.equal(from_raw, run(checkpoint_dir=full))
    # one more window: the modules' packed weights follow the version counter
    tr.train_window(A[:, 2:5], Bs[:, 2:5])
    later = str(tmp_path / "later")
    CK.save_trainer(tr, "latest", later)
    after = run(netG=tr.ema_generators())
    assert torch.equal(after, run(checkpoint_dir=later, weights="ema")), "the averaged modules ran on stale packed weights"
    assert not torch.equal(after, from_modules)
    with pytest.raises(ValueError, match="weights"):
        VideoTranslator(dev, 64, 128, checkpoint_dir=full, weights="bogus", **kw)
    with pytest.raises(FileNotFoundError, match="G0_ema"):
        VideoTranslator(dev, 64, 128, checkpoint_dir=raw_only, weights="ema", **kw)
