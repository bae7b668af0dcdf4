"""CPU side of the training schedule (ir2rgb_amd.schedule, ir2rgb_amd.losslog, ir2rgb_amd.training): hand-computed tables of
the learning-rate decay, the sequence-length and training-batch growth, resume points against the uninterrupted schedule, the
step accounting against a literal transcription of the reference's loop with the model calls removed, the loss log's
argument refusals before any launch and its entry point in every table, and the golden generator's source."""
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ir2rgb_loss_log_push"


def sched(**kw):
    from ir2rgb_amd.schedule import TrainingSchedule
    return TrainingSchedule(**kw)


# ---------------------------------------------------------------------------------------------
# tables
# ---------------------------------------------------------------------------------------------
def test_lr_decay_table():
    s = sched(lr=2e-4, niter=10, niter_decay=10)
    for e in range(1, 11):
        assert s.lr_after(e) == 2e-4
    # base_model.py:95, evaluated in Python floats as the reference evaluates it; tolerance 0
    for e in range(11, 21):
        assert s.lr_after(e) == 2e-4 * (1 - (e - 10) / 10)
    assert math.isclose(s.lr_after(11), 1.8e-4, rel_tol=1e-15) and s.lr_after(15) == 1e-4 and s.lr_after(20) == 0.0
    assert s.last_epoch == 20


def test_sequence_length_table():
    s = sched(n_frames_total=30, niter_step=5, n_input_gen_frames=3, seq_len_max=200)
    assert [s.n_frames_total_after(e) for e in (1, 4, 5, 9, 10, 14, 15, 20)] == [30, 30, 60, 60, 120, 120, 126, 126]
    s = sched(n_frames_total=30, niter_step=5, n_input_gen_frames=3, seq_len_max=40)
    assert [s.n_frames_total_after(e) for e in (1, 4, 5, 10, 15, 20)] == [30, 30, 38, 38, 38, 38]
    # the value is carried, not recomputed: a run that is already at the cap stays there
    assert s.n_frames_total_after(10, current=38) == 38 and s.n_frames_total_after(7, current=30) == 30


def test_training_batch_table():
    s = sched(max_frames_per_gpu=4, max_frames_backpropagate=4, n_frames_total=30)
    assert s.initial_training_batch() == (4, 1, 4)                     # generator.py:53-56: n_frames_load 4 from the start
    assert [s.training_batch_after(r) for r in range(4)] == [(4, 1), (4, 2), (4, 4), (4, 4)]
    # nfl // ceil(nfl / nfb): 3 frames loaded, 2 allowed -> two chunks -> 1 frame each
    s = sched(max_frames_per_gpu=3, max_frames_backpropagate=2, n_frames_total=30)
    assert s.update_training_batch(3, 1, 3, 1) == (3, 3 // math.ceil(3 / 2), 3) == (3, 1, 3)
    # frames per GPU below the maximum double per call (base_model.py:117-119)
    s = sched(max_frames_per_gpu=4, max_frames_backpropagate=4, n_frames_total=1)
    assert s.initial_training_batch() == (1, 1, 1)
    assert [s.training_batch_after(r) for r in range(4)] == [(1, 1), (2, 1), (4, 2), (4, 4)]


def test_fix_global_rule():
    s = sched(n_scales_spatial=2, niter_fix_global=3)
    assert [s.fix_global_ends(e) for e in (1, 2, 3, 4)] == [False, False, True, False] and s.fix_global_at_start()
    assert not sched(n_scales_spatial=1, niter_fix_global=3).fix_global_ends(3)
    assert not sched(n_scales_spatial=1, niter_fix_global=3).fix_global_at_start()
    assert not sched(n_scales_spatial=2, niter_fix_global=0).fix_global_ends(0)


def test_options_are_checked():
    with pytest.raises(TypeError):
        sched(n_iter=3)
    for bad in (dict(niter_step=0), dict(print_freq=0), dict(niter=-1), dict(niter=0, niter_decay=0), dict(seq_len_max=0)):
        with pytest.raises(ValueError):
            sched(**bad)


# ---------------------------------------------------------------------------------------------
# resume points
# ---------------------------------------------------------------------------------------------
def test_resume_equals_the_uninterrupted_schedule():
    """For every start_epoch the state init_params sets up (models.py:62-78) is the one an uninterrupted run holds at the
    start of that epoch.  The one exception is the reference's own: the resume calls update_learning_rate for
    start_epoch > niter (models.py:70-72), the loop only after an epoch > niter (:114-116).  At start_epoch = niter + 1 = 11
    the resumed run has therefore already assigned the rate -- still the undecayed value, lr * (1 - 0 / niter_decay) -- to
    optimizer_G and optimizer_D, one epoch before the uninterrupted run does; the value is the same, what differs is that
    the assignment has happened (which is what drops TTUR's factors under lr_policy="reference")."""
    s = sched(lr=2e-4, niter=10, niter_decay=10, niter_step=5, niter_fix_global=3, n_scales_spatial=2, n_frames_total=30,
              max_frames_per_gpu=4, max_frames_backpropagate=4, seq_len_max=200)
    run = s.start(7)
    at_start = {}
    while run.epoch <= s.last_epoch + 1:
        at_start[run.epoch] = (run.training_state(), run.lr_applied)
        s.end_epoch(run)
    assert at_start[1][0] == (2e-4, 30, 4, 1, True) and at_start[4][0][4] is False and at_start[3][0][4] is True
    assert at_start[21][0] == (0.0, 126, 4, 4, False)
    for start_epoch in range(1, 22):
        for epoch_iter in (0, 3):
            if (start_epoch, epoch_iter) == (1, 0):
                continue                  # (that is a fresh run)
            r = s.start(7, start_epoch, epoch_iter)
            assert r.training_state() == at_start[start_epoch][0], start_epoch
            if start_epoch == 11:
                assert r.lr_applied and not at_start[11][1] and r.lr == at_start[11][0][0] == 2e-4
            else:
                assert r.lr_applied == at_start[start_epoch][1], start_epoch
            # models.py:89-90
            assert r.total_steps == ((start_epoch - 1) * 7 + epoch_iter) // s.print_freq * s.print_freq


# ---------------------------------------------------------------------------------------------
# step accounting
# ---------------------------------------------------------------------------------------------
def reference_loop(n_sequences, niter, niter_decay, print_freq, save_latest_freq, save_epoch_freq, start_epoch=1, epoch_iter=0):
    """train_vid2vid.py:37-151 and models.py:88-110 with the model calls removed, batch size 1.  -> the list of
    ("print", epoch, epoch_iter) / ("save_latest", epoch, total_steps, iter.txt) / ("save_epoch", epoch, total_steps,
    iter.txt) events, and the counters as the loop leaves them."""
    events = []
    batch_size = 1
    dataset_size = n_sequences
    data_loader = list(range(n_sequences))
    total_steps = (start_epoch - 1) * len(data_loader) + epoch_iter                 # models.py:89
    total_steps = total_steps // print_freq * print_freq                           # models.py:90
    for epoch in range(start_epoch, niter + niter_decay + 1):                      # train_vid2vid.py:37
        for idx, video in enumerate(data_loader, start=epoch_iter):                # :39
            total_steps += batch_size                                              # :42
            epoch_iter += batch_size                                               # :43
            if total_steps % print_freq == 0:                                      # :119
                events.append(("print", epoch, epoch_iter))
            if total_steps % save_latest_freq == 0:                                # :139, models.py:98-102
                events.append(("save_latest", epoch, total_steps, (epoch, epoch_iter)))
            if epoch_iter > dataset_size - batch_size:                             # :140-142
                epoch_iter = 0
                break
        if epoch % save_epoch_freq == 0:                                           # :149, models.py:104-110
            events.append(("save_epoch", epoch, total_steps, (epoch + 1, 0)))
    return events, (epoch + 1, epoch_iter, total_steps)


def schedule_loop(s, n_sequences, start_epoch=1, epoch_iter=0):
    """The same run through TrainingSchedule.start / step / end_epoch, as ir2rgb_amd.training.fit drives it."""
    st = s.start(n_sequences, start_epoch, epoch_iter)
    events = []
    while st.epoch <= s.last_epoch:
        for _ in range(n_sequences):
            evs, over = s.step(st)
            events += evs
            if over:
                break
        events += s.end_epoch(st)[0]
    return events, (st.epoch, st.epoch_iter, st.total_steps)


def test_step_accounting_against_the_transcribed_loop():
    s = sched(niter=1, niter_decay=1, print_freq=2, save_latest_freq=4)
    got, left = schedule_loop(s, 3)
    want, want_left = reference_loop(3, 1, 1, 2, 4, 1)
    assert got == want and left == want_left
    assert want == [("print", 1, 2), ("save_epoch", 1, 3, (2, 0)), ("print", 2, 1), ("save_latest", 2, 4, (2, 1)), ("print", 2, 3),
                    ("save_epoch", 2, 6, (3, 0))]
    # the run of tests/test_schedule_gpu.py's fit test, and resumes into the middle of an epoch
    for n, niter, decay, pf, sf, se in ((2, 1, 2, 2, 3, 1), (5, 2, 3, 3, 4, 2), (1, 2, 1, 1, 1, 1)):
        s = sched(niter=niter, niter_decay=decay, print_freq=pf, save_latest_freq=sf, save_epoch_freq=se)
        assert schedule_loop(s, n) == reference_loop(n, niter, decay, pf, sf, se)
        for start_epoch in range(1, niter + decay + 1):
            for epoch_iter in range(0, n + 1):
                assert schedule_loop(s, n, start_epoch, epoch_iter) == \
                    reference_loop(n, niter, decay, pf, sf, se, start_epoch, epoch_iter), (n, start_epoch, epoch_iter)


def test_print_line_has_the_reference_shape():
    from ir2rgb_amd.training import format_errors, loss_names
    line = format_errors(3, 17, {"G_GAN": 1.23456, "D_fake": 0.5, "W": 0.0, "G_VGG": 0}, 0.0421)
    assert line == "(epoch: 3, iters: 17, time: 0.042) D_fake: 0.500 G_GAN: 1.235 "       # sorted, zeros left out
    names = loss_names(2)
    assert len(names) == len(set(names)) == 21 and {"G", "D", "D_T1", "G_T_GAN_Feat1", "F_Warp"} <= set(names)


# ---------------------------------------------------------------------------------------------
# the loss log's entry point and its refusals
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from ir2rgb_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.lib()


def test_entry_point_is_present_everywhere(lib):
    import ir2rgb_amd
    from ir2rgb_amd import _lib, fastbind, losslog, schedule, training
    header = open(os.path.join(ROOT, "include", "ir2rgb_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(" % NAME, header)
    assert NAME in _lib.PROTOTYPES and NAME in fastbind.wrappable()
    assert getattr(lib, NAME) is getattr(lib.fast_module, NAME)
    assert os.path.exists(os.path.join(ROOT, "ir2rgb_amd", "csrc", "loss_log.hip"))
    assert ir2rgb_amd.LossLog is losslog.LossLog and ir2rgb_amd.fit is training.fit
    assert ir2rgb_amd.TrainingSchedule is schedule.TrainingSchedule
    # the state block the Python side reads is the header's struct
    import ctypes
    m = re.search(r"#define\s+IR2RGB_LOSS_LOG_SLOTS\s+(\d+)", header)
    assert int(m.group(1)) == losslog.MAX_NAMES == 32
    assert ctypes.sizeof(_lib.LossLogState) == 8 * (2 * 32 + 2)
    assert _lib.LossLogState.skipped.offset == 512 and _lib.LossLogState.count.offset == 520
    m = re.search(r"#define\s+IR2RGB_LOSS_LOG_ABSENT\s+\((-[0-9.e+]+)f\)", header)
    assert float(np.float32(float(m.group(1)))) == losslog.ABSENT and np.isfinite(losslog.ABSENT)


def test_loss_log_refusals_before_any_launch(lib):
    """IR2RGB_EINVAL (-1) / IR2RGB_EALIGN (-3) through both bindings with nothing launched (no GPU here: the addresses
    are host memory that is never dereferenced as device memory)."""
    import ctypes
    import torch
    from ir2rgb_amd import losslog
    fast, handle = lib.fast_module, lib.ctypes_handle
    buf = torch.zeros(4096, dtype=torch.float64)
    p = buf.data_ptr()
    srcs = (ctypes.c_void_p * 40)(*([p] * 40))
    opts = (ctypes.c_void_p * 9)(*([p] * 9))
    sa, oa = ctypes.addressof(srcs), ctypes.addressof(opts)
    full = 0xFFFFFFFF

    def both(*args):
        a, b = getattr(fast, NAME)(*args), getattr(handle, NAME)(*args)
        assert a == b
        return a

    assert both(sa, full, 33, p, 4, p, None, 0, None) == -1            # 33 sources
    assert both(sa, full, -1, p, 4, p, None, 0, None) == -1
    assert both(sa, 0b11, 2, p, 0, p, None, 0, None) == -1             # capacity 0
    assert both(sa, 0b11, 2, p, -5, p, None, 0, None) == -1
    assert both(None, 0b11, 2, p, 4, p, None, 0, None) == -1           # no table
    assert both(sa, 0b11, 2, None, 4, p, None, 0, None) == -1          # no ring
    assert both(sa, 0b11, 2, p, 4, None, None, 0, None) == -1          # no state
    assert both(sa, 0b111, 2, p, 4, p, None, 0, None) == -1            # a slot past the sources
    srcs[1] = None
    assert both(sa, 0b11, 2, p, 4, p, None, 0, None) == -1             # a null source that is marked present
    srcs[1] = p + 2
    assert both(sa, 0b11, 2, p, 4, p, None, 0, None) == -3             # a misaligned one
    srcs[1] = p
    assert both(sa, 0b11, 2, p, 4, p, None, 1, None) == -1             # optimizers announced, none given
    assert both(sa, 0b11, 2, p, 4, p, oa, 9, None) == -1
    opts[2] = None
    assert both(sa, 0b11, 2, p, 4, p, oa, 3, None) == -1
    opts[2] = p + 4
    assert both(sa, 0b11, 2, p, 4, p, oa, 3, None) == -3
    assert both(sa, 0b11, 2, p + 2, 4, p, None, 0, None) == -3 and both(sa, 0b11, 2, p, 4, p + 4, None, 0, None) == -3
    # the Python side refuses the same before it touches a device
    for n, cap in ((33, 4), (0, 4), (2, 0), (2, -1), (2, True), (2, 1.5)):
        with pytest.raises(ValueError):
            losslog.check_arguments(n, cap)
    losslog.check_arguments(32, 1)
    with pytest.raises(ValueError, match="GPU only"):
        losslog.LossLog("cpu", ["G"])
    with pytest.raises(ValueError):
        losslog.LossLog("cpu", [f"t{i}" for i in range(33)])
    with pytest.raises(ValueError):
        losslog.LossLog("cpu", ["G", "G"])


def test_trainer_options_exist():
    from ir2rgb_amd import vid2vid as V
    assert V.DEFAULTS["niter_fix_global"] == 0 and V.DEFAULTS["TTUR"] is False and V.DEFAULTS["lr_policy"] == "reference"
    for name in ("update_fixed_params", "update_learning_rate", "update_training_batch", "attach_schedule"):
        assert callable(getattr(V.Vid2VidTrainer, name))
    from ir2rgb_amd.flatgrads import FlatGrads
    assert callable(FlatGrads.close)


def test_golden_generator_subclasses_the_window_generator():
    """tests/golden/make_schedule_goldens.py restates only the two finetune_all branches on top of
    make_window_goldens.RefModelG (it cannot be imported here: it imports the reference)."""
    src = open(os.path.join(ROOT, "tests", "golden", "make_schedule_goldens.py")).read()
    assert "import make_window_goldens" in src and re.search(r"class \w+\(RefModelG\)", src)
    assert "generator.py:64-72" in src and "generator.py:166-170" in src
    path = os.path.join(ROOT, "tests", "golden", "window_2scale_fixglobal_ngf64_64x128.npz")
    assert os.path.getsize(path) < 1 << 20
    g = np.load(path)
    assert int(g["n_windows"]) == 2 and int(g["n_scales_spatial"]) == 2 and int(g["ngf"]) == 64
    assert g["seq_A"].shape == (1, 4, 3, 64, 128) and not g["w0/G0/grad_norms"].any() and g["w0/G1/grad_norms"].any()
    assert any(k.startswith("floor/f16/w1/loss/") for k in g.files) and any(k.startswith("floor/bf16/G1/l2/") for k in g.files)


@pytest.mark.parametrize("ttur", [False, True])
@pytest.mark.parametrize("policy", ["reference", "all"])
def test_between_epoch_methods_with_torch_adam(policy, ttur):
    """The trainer's optimizer bookkeeping needs no kernel with fused_adam=False: built on the CPU, no window is run.
    (tests/test_schedule_gpu.py repeats this with FusedAdam.)"""
    import torch
    from ir2rgb_amd import vid2vid as V
    tr = V.Vid2VidTrainer(torch.device("cpu"), n_scales_spatial=2, first_layer_gen_filters=32, build_flow_net=False, fused_adam=False,
                          batched_repack=False, niter_fix_global=1, TTUR=ttur, lr_policy=policy)
    rate = lambda o: o.param_groups[0]["lr"]  # noqa: E731
    lr, (fg, fd) = 2e-4, ((0.5, 2.0) if ttur else (1.0, 1.0))
    fine = [id(p) for p in tr.netG[1].parameters()]
    assert [id(p) for p in tr.grads_G.params] == fine == [id(p) for p in tr.optimizer_G.param_groups[0]["params"]]
    assert (rate(tr.optimizer_G), rate(tr.optimizer_D)) == (lr * fg, lr * fd) and all(rate(o) == lr for o in tr.optimizer_D_T)
    tr.attach_schedule(sched(niter=10, niter_decay=10, lr=lr, n_scales_spatial=2, niter_fix_global=1))
    new = tr.update_learning_rate(15)
    assert new == 1e-4
    if policy == "reference":
        assert (rate(tr.optimizer_G), rate(tr.optimizer_D)) == (new, new) and all(rate(o) == lr for o in tr.optimizer_D_T)
    else:
        assert (rate(tr.optimizer_G), rate(tr.optimizer_D)) == (new * fg, new * fd) and all(rate(o) == new for o in tr.optimizer_D_T)
    old = tr.grads_G
    tr.update_fixed_params()
    every = [id(p) for g in tr.netG for p in g.parameters()]
    assert tr.finetune_all and [id(p) for p in tr.grads_G.params] == every == [id(p) for p in tr.optimizer_G.param_groups[0]["params"]]
    assert tr.grads_G is not old and not tr.optimizer_G.state
    keep = policy == "all"
    assert rate(tr.optimizer_G) == new * (fg if keep else 1.0)
    assert tuple(tr.optimizer_G.param_groups[0]["betas"]) == ((0.0, 0.9) if ttur and keep else (0.5, 0.999))
    with pytest.raises(ValueError):
        V.Vid2VidTrainer(torch.device("cpu"), build_flow_net=False, fused_adam=False, lr_policy="linear")
