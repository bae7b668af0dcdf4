"""A training run: the epoch -> sequence -> window loop of train_vid2vid.py:37-151 around ``Vid2VidTrainer.train_window``.

What happens between windows and between epochs is ``ir2rgb_amd.schedule.TrainingSchedule``'s host arithmetic; the loss
record is ``ir2rgb_amd.losslog.LossLog``'s, on the device.  Nothing inside the loop synchronises with the GPU except
``LossLog.read`` every ``print_freq`` sequences and the checkpoints; the visualiser (``ir2rgb_amd.visuals.Snapshots``)
composes its panels on the device and writes its files one snapshot late, when the copy has long finished.  Not carried
over: ``sparse_D``, ``pool_size``, ``max_t_step``, and optimizer state in checkpoints (the reference saves none either: a
resumed run restarts Adam's moments, models/utils.py:6-9).
"""
import time

from . import checkpoint
from .frames import WindowSlicer
from .losslog import LossLog

# every term train_window can return with two temporal scales (the reference's loss_names / loss_names_T with the scale
# appended, and the totals its losses_G / losses_D lists hold): 21 of the log's 32 slots.  ``grad_norms``: also the gradient
# norms a guarded trainer (``max_grad_norm``) returns, one per optimizer: 25 slots
def loss_names(t_scales, grad_norms=False):
    names = ["G", "D"] + [f"D_T{s}" for s in range(t_scales)]
    names += ["G_VGG", "G_GAN", "G_GAN_Feat", "D_real", "D_fake", "G_Warp", "F_Flow", "F_Warp", "W"]
    for s in range(t_scales):
        names += [f"G_T_GAN{s}", f"G_T_GAN_Feat{s}", f"D_T_real{s}", f"D_T_fake{s}"]
    if grad_norms:
        names += ["GN_G", "GN_D"] + [f"GN_D_T{s}" for s in range(t_scales)]
    return names


def format_errors(epoch, i, errors, t):
    """Visualizer.print_current_errors (util/visualizer.py:100-106)."""
    message = "(epoch: %d, iters: %d, time: %.3f) " % (epoch, i, t)
    for k, v in sorted(errors.items()):
        if v != 0:
            message += "%s: %.3f " % (k, v)
    return message


def _in_frame_history(trainer, t):
    """Is ``t`` a view of one of the trainer's preallocated ``FrameHistory`` buffers (which later pushes overwrite)?"""
    bufs = [h.buf for h in trainer.hist.values() if h.buf is not None]
    return any(b.untyped_storage().data_ptr() == t.untyped_storage().data_ptr() for b in bufs)


def fit(trainer, sequences, schedule, save_dir=None, log=print, loss_log=None, continue_train=False, events=None,
        snapshots=None):
    """Trains ``trainer`` through ``schedule``'s epochs.

    ``sequences``: ``len()``, ``seq_len_max`` and ``sequence(index, n_frames_total) -> (ir, rgb)``, device tensors
    ``[1, T, C, H, W]`` with T <= n_frames_total + tG - 1 frames (decoding and scaling files is the caller's business:
    ``frames.scaled_sequence``).  ``save_dir``: where ``checkpoint.save_trainer`` writes at the schedule's save points
    (None: nowhere).  ``loss_log``: a ``LossLog`` (default: one over every term of the trainer).  ``continue_train``:
    resume from ``save_dir``'s ``latest`` networks and ``iter.txt`` (models.py:62-78).  ``events``: a list that receives
    the schedule's ("print" | "save_latest" | "save_epoch", ...) tuples as they happen.  ``snapshots``: a
    ``visuals.Snapshots``; after every sequence that brings ``total_steps`` to a multiple of its ``freq``
    (train_vid2vid.py:46, :131-136) it draws the last window and the sequence's first generated frame.  Without one the loop
    issues no launch and makes no allocation for it.
    -> (epoch, epoch_iter, total_steps) as the loop leaves them."""
    n = len(sequences)
    if n < 1:
        raise ValueError("fit: no sequences")
    if schedule.seq_len_max != sequences.seq_len_max:
        raise ValueError(f"fit: schedule.seq_len_max {schedule.seq_len_max} differs from the sequences' {sequences.seq_len_max}")
    for k in ("n_input_gen_frames", "n_scales_spatial", "niter_fix_global", "max_frames_per_gpu"):
        if getattr(schedule, k) != trainer.opt[k]:
            raise ValueError(f"fit: {k} is {getattr(schedule, k)!r} in the schedule and {trainer.opt[k]!r} in the trainer")
    trainer.attach_schedule(schedule)
    start_epoch, epoch_iter = 1, 0
    if continue_train:
        if save_dir is None:
            raise ValueError("fit: continue_train needs save_dir")
        start_epoch, epoch_iter = checkpoint.load_trainer(trainer, "latest", save_dir, log)
        log("Resuming from epoch %d at iteration %d" % (start_epoch, epoch_iter))
    st = schedule.start(n, start_epoch, epoch_iter)
    if st.lr_applied:
        trainer.update_learning_rate(start_epoch - 1)
    if not st.fix_global:
        trainer.update_fixed_params()
    n_frames_load = trainer.update_training_batch(st.ratio, resume=True)
    assert (n_frames_load, trainer.opt["n_frames_bp"]) == (st.n_frames_load, st.n_frames_bp)
    if loss_log is None:
        loss_log = LossLog(trainer.device, loss_names(trainer.t_scales, grad_norms=trainer.grad_guards is not None))
    tG = schedule.n_input_gen_frames
    totals = {"G", "D"} | {f"D_T{s}" for s in range(trainer.t_scales)}
    opt = trainer.opt

    def emit(evs):
        for ev in evs:
            if events is not None:
                events.append(ev)
            if ev[0] == "print":
                r = loss_log.read()
                errors = {k: v for k, v in r["last"].items() if k not in totals}     # (the terms; the totals are history())
                t = (time.time() - t_print[0]) / schedule.print_freq
                log(format_errors(ev[1], ev[2], errors, t) + (f"skipped: {r['skipped']} " if r["skipped"] else ""))
            elif ev[0] == "save_latest":
                log(f"saving the latest model (epoch {ev[1]}, total_steps {ev[2]})")
                if save_dir is not None:
                    checkpoint.save_trainer(trainer, "latest", save_dir, *ev[3])
            elif ev[0] == "save_epoch":
                log(f"saving the model at the end of epoch {ev[1]}, iters {ev[2]}")
                if save_dir is not None:
                    checkpoint.save_trainer(trainer, "latest", save_dir)
                    checkpoint.save_trainer(trainer, ev[1], save_dir, *ev[3])

    t_print = [time.time()]
    while st.epoch <= schedule.last_epoch:
        epoch_start = time.time()
        for index in range(n):
            if st.total_steps % schedule.print_freq == 0:
                t_print[0] = time.time()
            ir, rgb = sequences.sequence(index, st.n_frames_total)
            b, t, c, h, w = ir.shape
            slicer = WindowSlicer(ir.reshape(b, t * c, h, w), rgb.reshape(b, t * rgb.shape[2], h, w), tG, n_frames_load,
                                  opt["input_nc"], opt["output_nc"])
            trainer.reset_sequence()
            save_fake = snapshots is not None and snapshots.due(st.total_steps + 1)      # (schedule.step: one per sequence)
            fake_B_first = None
            for i, (input_A, input_B) in enumerate(slicer):
                out = trainer.train_window(input_A, input_B)
                if trainer.grad_guards is None:
                    loss_log.push(out, trainer.loss_scaler)
                else:           # guarded steps: a skipped window counts with or without a scaler
                    loss_log.push(out, trainer.loss_scaler, trainer.decided_optimizers())
                if save_fake and i == 0:       # the first generated image of this sequence (train_vid2vid.py:113-114)
                    fake_B_first = trainer.last_outputs[0][0, 0]
                    if _in_frame_history(trainer, fake_B_first):
                        fake_B_first = fake_B_first.clone()
            evs, over = schedule.step(st)
            emit(evs)
            if fake_B_first is not None:        # queued before the next window: FlowNet2's next replay overwrites flow_ref
                snapshots.take(trainer, st.epoch, fake_B_first)
            if over:
                break
        log(f"End of epoch {st.epoch} / {schedule.last_epoch} \t Time Taken: {time.time() - epoch_start} sec")
        epoch = st.epoch
        evs, changes = schedule.end_epoch(st)
        emit(evs)
        if "lr" in changes:
            old = trainer.optimizer_G.param_groups[0]["lr"]
            log("update learning rate: %f -> %f" % (old, trainer.update_learning_rate(epoch)))
        if "training_batch" in changes:
            n_frames_load = trainer.update_training_batch(st.ratio)
            assert (n_frames_load, opt["n_frames_bp"]) == changes["training_batch"]
        if changes.get("update_fixed_params"):
            trainer.update_fixed_params()
            log("------------ Now finetuning all scales -----------")
    if snapshots is not None:
        snapshots.flush()
    return st.epoch, st.epoch_iter, st.total_steps
